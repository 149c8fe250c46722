"""GPU: moge_amd.optim.AdamW (csrc/optim.hip) on the shared fixture of tests/optim_fixtures.py against the float64 restatement of
tests/optim_reference.py, which tests/test_optim_reference_cpu.py pins to torch's own classes.

Accuracy is measured per tensor as max |x - x64| / max |x64| and bounded by max(4 x the same error of torch's fp32 CPU run, t 2^-23) after
step t (R.bound): a different but equally long chain of fp32 roundings, and a floor where torch happens to be exact.  Measured on an MI355X,
worst tensor over the six steps with a clip at 1 (error / bound): p 4.6e-7 / 1.8e-6, exp_avg 6.0e-6 / 1.4e-5 (the 1-element tensor, where m
cancels), exp_avg_sq 2.4e-7 / 9.6e-7, ema 3.7e-7 / 1.5e-6; grad_norm equal to the float64 reference's to the last bit.
The fixture's small gradients have norm 1.58, so a clip at 1 engages on every step: the accuracy test also runs with a clip at 2, where every
other step goes unclipped."""
import pytest
import torch

import moge_amd.optim as M
from tests import optim_fixtures as F
from tests import optim_reference as R

pytestmark = pytest.mark.gpu

C = F.C
CLIP_EMA = dict(max_grad_norm=1.0, ema_decay=0.999)
SCALE = dict(init_scale=4.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2)


@pytest.fixture(scope="module", autouse=True)
def _needs_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


class Run:
    """The fixture's tensors on the GPU under one optimizer; everything is read back in fixture order."""

    def __init__(self, aligned_view=False, only=None, **kw):
        self.params = F.initial(device="cuda", aligned_view=aligned_view)
        self.only = only
        if only is None:
            groups = F.param_groups(self.params)
        else:
            groups = [{"params": [self.params[F.INDEX[only]]], **F.GROUPS[F.GROUP_OF[F.INDEX[only]]]}]
        self.opt = M.AdamW(groups, **kw)

    def step(self, t, scale=1.0, poison=None, **kw):
        for p, g in zip(self.params, F.gradients(t, device="cuda", scale=scale, poison=poison)):
            p.grad = g
        self.opt.step(**kw)

    def get(self, key):
        if key == "p":
            return self.params
        if key == "ema":
            order = F.group_order() if self.only is None else [F.INDEX[self.only]]
            out = [None] * len(self.params)
            for k, e in zip(order, self.opt.ema_parameters()):
                out[k] = e
            return out
        return [self.opt.state[p].get({"m": "exp_avg", "v": "exp_avg_sq"}[key]) if p in self.opt.state else None for p in self.params]

    def bits(self, keys=("p", "m", "v", "ema")):
        return {k: [None if x is None else x.detach().cpu().clone() for x in self.get(k)] for k in keys}

    def scalars(self):
        o = self.opt
        return [float(x) for x in (o.applied_steps, o.skipped_steps, o.found_nonfinite, o.grad_norm, o.scale, o.growth_tracker)]


def same(a, b, names=None):
    for key in a:
        for name, x, y in zip(F.NAMES, a[key], b[key]):
            if names is None or name in names:
                assert (x is None and y is None) or torch.equal(x.view(torch.int32), y.view(torch.int32)), (key, name)


def within(run, ref_snap, t32_snap, t, keys=("p", "m", "v", "ema"), report=None):
    """every tensor of `run` against the reference snapshot after step t (1-based)"""
    for key in keys:
        for name, x, x64, x32 in zip(F.NAMES, run.get(key), ref_snap[key], t32_snap[key]):
            err, bound = R.tensor_error(x, x64), R.bound(t, x32, x64)
            if report is not None and err >= report.get(key, (0.0,))[0]:
                report[key] = (err, bound, name, t)
            assert err <= bound, (t, key, name, err, bound)


# ---- accuracy ----
@pytest.mark.parametrize("max_grad_norm", [1.0, 2.0])
def test_every_step_follows_the_float64_reference(max_grad_norm):
    ref, t32 = R.standard("ref", max_grad_norm), R.standard("torch32", max_grad_norm)
    run = Run(max_grad_norm=max_grad_norm, ema_decay=0.999)
    worst = {}
    for t in range(F.T):
        run.step(t)
        within(run, ref[t], t32[t], t + 1, report=worst)
        norm = float(run.opt.grad_norm)
        worst["grad_norm"] = max(worst.get("grad_norm", (0.0,)), (abs(norm - ref[t]["grad_norm"]) / ref[t]["grad_norm"],))
        assert abs(norm - ref[t]["grad_norm"]) <= 1e-6 * ref[t]["grad_norm"], (t, norm, ref[t]["grad_norm"])
        assert float(run.opt.found_nonfinite) == 0.0 and float(run.opt.applied_steps) == t + 1
    print("measured (error, bound, tensor, step) of the worst tensor over the steps:", worst)
    assert float(run.opt.skipped_steps) == 0.0 and float(run.opt.scale) == 1.0


def test_first_applied_step_copies_p_into_the_ema():
    run = Run(**CLIP_EMA)
    before = [p.clone() for p in run.params]
    run.step(0)
    b = run.bits()
    same({"x": b["p"]}, {"x": b["ema"]})
    nograd = F.INDEX["nograd"]
    assert torch.equal(b["ema"][nograd], before[nograd].cpu()) and not torch.equal(b["p"][F.INDEX["c"]], before[F.INDEX["c"]].cpu())


# ---- bits ----
def test_two_runs_give_the_same_bits():
    out = []
    for _ in range(2):
        run = Run(**CLIP_EMA)
        for t in range(3):
            run.step(t)
        out.append((run.bits(), run.scalars()))
    same(out[0][0], out[1][0])
    assert out[0][1] == out[1][1]


@pytest.mark.parametrize("name", ["n5", "c_plus", "two_c", "matrix", "view"])
def test_a_tensor_alone_gives_the_bits_it_gives_inside_the_list(name):
    whole, alone = Run(ema_decay=0.999), Run(only=name, ema_decay=0.999)
    for t in range(2):
        whole.step(t)
        alone.step(t)
    same(whole.bits(), alone.bits(), names=[name])


def test_the_misaligned_view_gives_the_bits_of_an_aligned_tensor():
    view, flat = Run(**CLIP_EMA), Run(aligned_view=True, **CLIP_EMA)
    i = F.INDEX["view"]
    assert view.params[i].data_ptr() % 16 == 4 and flat.params[i].data_ptr() % 16 == 0
    for t in range(3):
        view.step(t, zero_grad=True)
        flat.step(t, zero_grad=True)
        assert float(view.opt.grad_norm) == float(flat.opt.grad_norm)
        assert not view.params[i].grad.any() and not flat.params[i].grad.any()
    same(view.bits(), flat.bits())


def test_a_side_stream_gives_the_default_stream_bits():
    main, side_run = Run(**CLIP_EMA), Run(**CLIP_EMA)
    side = torch.cuda.Stream()
    for t in range(2):
        main.step(t)
        for p, g in zip(side_run.params, F.gradients(t, device="cuda")):
            p.grad = g
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            side_run.opt.step()
        torch.cuda.current_stream().wait_stream(side)
    same(main.bits(), side_run.bits())
    assert main.scalars() == side_run.scalars()


def test_a_tensor_without_grad_stays_as_it_is():
    run = Run(**CLIP_EMA)
    i = F.INDEX["nograd"]
    before = run.params[i].clone()
    for t in range(2):
        run.step(t)
        assert run.params[i].grad is None
    b = run.bits()
    assert torch.equal(b["p"][i], before.cpu()) and torch.equal(b["ema"][i], before.cpu())
    assert not b["m"][i].any() and not b["v"][i].any()


def test_zero_grad_leaves_exact_zeros_in_the_same_storage():
    run = Run(**CLIP_EMA)
    plain = Run(**CLIP_EMA)
    run.step(0, zero_grad=True)
    plain.step(0)
    grads = [p.grad for p in run.params]
    ptrs = [None if g is None else g.data_ptr() for g in grads]
    for name, g in zip(F.NAMES, grads):
        assert g is None or (not g.any() and not torch.signbit(g).any()), name
    same(run.bits(), plain.bits())                                     # zeroing changes nothing else
    for p in run.params:                                               # the next backward accumulates into the same tensors
        if p.grad is not None:
            p.grad += 1.0
    run.opt.step(zero_grad=True)
    assert [None if p.grad is None else p.grad.data_ptr() for p in run.params] == ptrs
    assert all(p.grad is None or not p.grad.any() for p in run.params)
    assert all(plain.params[i].grad is None or plain.params[i].grad.any() for i in range(len(F.NAMES)) if plain.params[i].numel())


# ---- skips ----
@pytest.mark.parametrize("poison", [{"c_plus": (C, float("nan"))}, {"n1": (0, float("inf"))}], ids=["nan_in_the_tail", "inf_in_one_element"])
def test_a_nonfinite_gradient_skips_the_step(poison):
    at = {1: {"c_plus": (C, float("nan"))}}                            # the skipped step changes nothing: both cases share this reference
    ref, t32 = R.run_reference(steps=3, poison=at, **CLIP_EMA), R.run_torch(torch.float32, steps=3, poison=at, **CLIP_EMA)
    run = Run(**CLIP_EMA)
    run.step(0)
    before, counts = run.bits(), run.scalars()
    run.step(1, poison=poison, zero_grad=True)
    same(before, run.bits())                                           # p / m / v bit-unchanged, and without loss scaling the EMA too
    after = run.scalars()
    assert after[:3] == [counts[0], counts[1] + 1, 1.0] == [1.0, 1.0, 1.0]
    assert all(p.grad is None or not p.grad.any() for p in run.params)        # zero_grad still zeroes
    run.step(2)
    assert run.scalars()[:3] == [2.0, 1.0, 0.0]
    within(run, ref[2], t32[2], 3)                                     # bias corrections of step 2, not 3


def test_loss_scaling_follows_grad_scaler():
    kw = dict(steps=5, loss_scale=SCALE, poison={2: {"n1": (0, float("inf"))}}, **CLIP_EMA)
    ref, t32 = R.run_reference(**kw), R.run_torch(torch.float32, **kw)
    assert [s["scale"] for s in t32] == [s["scale"] for s in ref]
    run = Run(loss_scale=SCALE, **CLIP_EMA)
    assert float(run.opt.scale_loss(torch.ones((), device="cuda"))) == 4.0
    for t in range(5):
        before = run.bits() if t else None                             # the state exists after the first step
        run.step(t, scale=ref[t]["scale_before"], poison=kw["poison"].get(t))
        applied, skipped, found, norm, scale, tracker = run.scalars()
        assert (scale, tracker) == (ref[t]["scale"], ref[t]["tracker"]) == (t32[t]["scale"], t32[t]["tracker"]), t
        assert (applied, skipped, found) == (ref[t]["applied"], ref[t]["skipped"], float(ref[t]["found"])), t
        if t == 2:
            now = run.bits()
            same({k: before[k] for k in "pmv"}, {k: now[k] for k in "pmv"})
            for (name, _, kind), x, y, p in zip(F.TENSORS, before["ema"], now["ema"], before["p"]):       # the EMA is blended on the skipped step
                assert torch.equal(y, x if kind == "nograd" else 0.999 * x + (1 - 0.999) * p), name     # (a 1e-8 move is below fp32 for most elements)
            assert not torch.equal(before["ema"][F.INDEX["two_c"]], now["ema"][F.INDEX["two_c"]])
        else:
            assert abs(norm - ref[t]["grad_norm"]) <= 1e-6 * ref[t]["grad_norm"]
        within(run, ref[t], t32[t], t + 1)
    assert float(run.opt.scale_loss(torch.full((), 0.5, device="cuda"))) == 4.0


# ---- no host wait ----
def test_step_does_not_wait_for_the_device():
    run = Run(loss_scale=SCALE, **CLIP_EMA)
    grads = [F.gradients(t, device="cuda") for t in range(3)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for t in range(3):                                             # the first step makes the state; the later ones re-upload the table for new grads
            for p, g in zip(run.params, grads[t]):
                p.grad = g
            run.opt.step(zero_grad=(t == 1))
            run.opt.scale_loss(run.params[0].sum())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert run.scalars()[0] == 3.0


# ---- checkpoints ----
def test_state_dict_goes_to_torch_adamw_and_continues_there():
    ref, t32 = R.run_reference(steps=4), R.run_torch(torch.float32, steps=4)
    run = Run()
    for t in range(3):
        run.step(t)
    cpu = [p.detach().cpu().clone() for p in run.params]
    theirs = torch.optim.AdamW(F.param_groups(cpu), foreach=False)
    state = run.opt.state_dict()
    assert float(state["state"][0]["step"]) == 3.0 and state["state"][0]["step"].device.type == "cpu"
    theirs.load_state_dict(state)
    for p, g in zip(cpu, F.gradients(3)):
        p.grad = g
    theirs.step()
    run.step(3)
    for name, x, y, x64, x32 in zip(F.NAMES, run.params, cpu, ref[3]["p"], t32[3]["p"]):
        assert R.tensor_error(x, y) <= R.bound(4, x32, x64), name


def test_state_dict_comes_from_torch_adamw_and_continues_here():
    ref, t32 = R.run_reference(steps=4), R.run_torch(torch.float32, steps=4)
    cpu = F.initial()
    theirs = torch.optim.AdamW(F.param_groups(cpu), foreach=False)
    for t in range(3):
        for p, g in zip(cpu, F.gradients(t)):
            p.grad = g
        theirs.step()
    run = Run()
    for p, q in zip(run.params, cpu):
        p.copy_(q)
    run.opt.load_state_dict(theirs.state_dict())
    run.step(3)
    for p, g in zip(cpu, F.gradients(3)):
        p.grad = g
    theirs.step()
    assert float(run.opt.applied_steps) == 4.0
    for name, x, y, x64, x32 in zip(F.NAMES, run.params, cpu, ref[3]["p"], t32[3]["p"]):
        assert R.tensor_error(x, y) <= R.bound(4, x32, x64), name
    assert float(run.opt.state_dict()["state"][1]["step"]) == 4.0
