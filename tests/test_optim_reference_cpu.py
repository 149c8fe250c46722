"""CPU: the float64 restatement of the optimizer step (tests/optim_reference.py) against the real classes on the shared fixture, in float64:
torch.optim.AdamW(foreach=False), clip_grad_norm_, AveragedModel with the reference's avg_fn and torch.amp.GradScaler("cpu").  This pins the
reference the GPU tests compare with to torch itself."""
import pytest
import torch

from tests import optim_fixtures as F
from tests import optim_reference as R

TOL = 1e-12          # float64 rounding over a handful of operations and steps, by the per-tensor measure


def agree(ref, real):
    assert len(ref) == len(real)
    for t, (a, b) in enumerate(zip(ref, real)):
        for key in ("p", "m", "v", "ema"):
            if a[key] is None:
                assert b[key] is None
                continue
            for name, x, y in zip(F.NAMES, a[key], b[key]):
                assert x.shape == y.shape and R.tensor_error(x, y) <= TOL, (t, key, name, R.tensor_error(x, y))


def test_fixture_is_what_the_issue_lists():
    C = F.C
    sizes = [torch.Size(s).numel() for _, s, _ in F.TENSORS]
    for n in (1, 3, 4, 5, 63, 64, 65, C - 1, C, C + 1, 2 * C + 3, 63, 0, C + 2):
        assert n in sizes
    assert sum(sizes) < 10 * C and F.T == 6
    view = F.initial()[F.INDEX["view"]]
    assert view.storage_offset() == 1 and view.numel() == C + 2
    grads = [F.gradients(t) for t in range(F.T)]
    assert all(g[F.INDEX["nograd"]] is None for g in grads)
    big, small = float(grads[0][F.INDEX["c"]].abs().mean()), float(grads[1][F.INDEX["c"]].abs().mean())
    assert 5 < big < 12 and 0.005 < small < 0.012


def test_clip_adamw_ema_follow_torch():
    kw = dict(max_grad_norm=1.0, ema_decay=0.999)
    ref = R.run_reference(**kw)
    agree(ref, R.run_torch(torch.float64, **kw))
    norms = [s["grad_norm"] for s in ref]
    # gradients of 10 x randn clip hard; those of 0.01 x randn have norm 0.01 sqrt(24849) = 1.58 over this fixture, so max_grad_norm = 1 still
    # engages (mildly) and the unclipped branch is the run at max_grad_norm = 2 below
    assert all(n > 1000 for n in norms[0::2]) and all(1.5 < n < 1.65 for n in norms[1::2])
    assert ref[-1]["applied"] == F.T and ref[-1]["skipped"] == 0
    for name, p, e in zip(F.NAMES, ref[0]["p"], ref[0]["ema"]):
        assert torch.equal(p, e), name                                                     # AveragedModel's copy at n_averaged == 0


def test_without_clip_or_ema_follows_torch():
    agree(R.run_reference(steps=3), R.run_torch(torch.float64, steps=3))


def test_clip_that_engages_on_every_other_step_follows_torch():
    kw = dict(max_grad_norm=2.0, ema_decay=0.999)
    agree(R.run_reference(**kw), R.run_torch(torch.float64, **kw))


def test_nan_step_is_skipped_as_train_py_skips_it():
    poison = {2: {"c_plus": (F.C, float("nan"))}}
    kw = dict(max_grad_norm=1.0, ema_decay=0.999, poison=poison)
    ref = R.run_reference(**kw)
    agree(ref, R.run_torch(torch.float64, **kw))
    assert ref[2]["found"] and ref[2]["applied"] == 2 and ref[2]["skipped"] == 1 and ref[-1]["applied"] == F.T - 1
    for key in ("p", "m", "v", "ema"):
        for x, y in zip(ref[1][key], ref[2][key]):
            assert torch.equal(x, y)


def test_loss_scaling_follows_grad_scaler():
    scale = dict(init_scale=4.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2)
    poison = {2: {"n1": (0, float("inf"))}}
    kw = dict(steps=5, max_grad_norm=1.0, ema_decay=0.999, loss_scale=scale, poison=poison)
    ref, real = R.run_reference(**kw), R.run_torch(torch.float64, **kw)
    agree(ref, real)
    assert [s["scale"] for s in ref] == [s["scale"] for s in real] == [4.0, 8.0, 4.0, 4.0, 8.0]
    assert [s["tracker"] for s in ref] == [s["tracker"] for s in real] == [1, 0, 0, 1, 0]
    assert [s["scale_before"] for s in ref] == [4.0, 4.0, 8.0, 4.0, 4.0]
    for x, y in zip(ref[1]["p"], ref[2]["p"]):
        assert torch.equal(x, y)                                                           # the poisoned step is skipped ...
    for (name, _, kind), x, y in zip(F.TENSORS, ref[1]["ema"], ref[2]["ema"]):
        assert torch.equal(x, y) == (x.numel() == 0 or kind == "nograd"), name              # ... and the EMA still blends


def test_inf_without_loss_scaling_is_the_documented_difference():
    """train.py:341 checks isnan only: an inf gradient reaches clip_grad_norm_ there (clip_coef 0, 0 * inf = NaN parameters).  The restatement,
    like moge_amd.optim, skips the step."""
    poison = {1: {"n1": (0, float("inf"))}}
    ref = R.run_reference(steps=2, max_grad_norm=1.0, poison=poison)
    real = R.run_torch(torch.float64, steps=2, max_grad_norm=1.0, poison=poison)
    assert ref[1]["found"] and all(torch.equal(x, y) for x, y in zip(ref[0]["p"], ref[1]["p"]))
    assert not torch.isfinite(real[1]["p"][F.INDEX["n1"]]).all()
