"""CPU: the host side of moge_amd.optim - what the constructor refuses, build_optimizer / build_lr_scheduler on the reference's config blocks
(tests/golden/optim_v2_blocks.json: the `optimizer` and `lr_scheduler` blocks of configs/train/v2.json), the state-dict exchange with
torch.optim.AdamW, and that step() refuses CPU tensors.  No GPU call is made here."""
import json
import os

import pytest
import torch

import moge_amd.optim as M
from tests import optim_fixtures as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCKS = json.load(open(os.path.join(ROOT, "tests", "golden", "optim_v2_blocks.json")))


def test_constructor_takes_what_torch_takes():
    params = F.initial()
    a = M.AdamW(params, lr=3e-4, betas=(0.8, 0.9), eps=1e-6, weight_decay=0.1, max_grad_norm=1.0, ema_decay=0.999, loss_scale=dict(init_scale=4.0))
    g = a.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"]) == (3e-4, (0.8, 0.9), 1e-6, 0.1) and len(g["params"]) == len(params)
    assert a.loss_scale == dict(init_scale=4.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000) and a.max_grad_norm == 1.0 and a.ema_decay == 0.999
    b = M.AdamW(F.param_groups(params))
    assert [x["lr"] for x in b.param_groups] == [1e-4, 1e-5] and b.param_groups[1]["betas"] == (0.8, 0.99) and b.param_groups[1]["weight_decay"] == 0.0
    assert set(torch.optim.AdamW([torch.zeros(1)]).param_groups[0]) <= set(b.param_groups[0])          # every key torch's own step reads
    assert b.max_grad_norm is None and b.ema_decay is None and b.loss_scale is None
    assert M.LOSS_SCALE_DEFAULTS == dict(init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000)
    assert b._chunks == sum(-(-p.numel() // M.CHUNK) for p in params)


@pytest.mark.parametrize("make, reason", [
    (lambda: M.AdamW([torch.zeros(4)], amsgrad=True), "amsgrad"),
    (lambda: M.AdamW([torch.zeros(4)], maximize=True), "maximize"),
    (lambda: M.AdamW([{"params": [torch.zeros(4)], "amsgrad": True}]), "amsgrad"),
    (lambda: M.AdamW([torch.zeros(4, dtype=torch.float16)]), "fp32"),
    (lambda: M.AdamW([torch.zeros(4, dtype=torch.float64)]), "fp32"),
    (lambda: M.AdamW([torch.zeros(4, 6).t()]), "contiguous"),
    (lambda: M.AdamW([torch.zeros(4), torch.zeros(4, device="meta")]), "two devices"),
    (lambda: M.AdamW([torch.zeros(4)], betas=(1.0, 0.999)), "betas"),
    (lambda: M.AdamW([torch.zeros(4)], lr=-1.0), "lr"),
    (lambda: M.AdamW([torch.zeros(4)], max_grad_norm=-1.0), "max_grad_norm"),
    (lambda: M.AdamW([torch.zeros(4)], ema_decay=1.0), "ema_decay"),
    (lambda: M.AdamW([torch.zeros(4)], loss_scale=dict(scale=2.0)), "loss_scale"),
    (lambda: M.AdamW([torch.zeros(4)], loss_scale=dict(growth_interval=0)), "growth_interval"),
    (lambda: M.AdamW([{"params": [torch.zeros(1)]} for _ in range(M.MAX_GROUPS + 1)]), "parameter groups"),
])
def test_constructor_refusals(make, reason):
    with pytest.raises(ValueError, match=reason):
        make()


def test_step_refuses_cpu_tensors_with_the_standard_message():
    p = torch.zeros(8)
    p.grad = torch.ones(8)
    opt = M.AdamW([p])
    with pytest.raises(RuntimeError, match="GPU tensors only") as e:
        opt.step()
    assert "moge_amd.optim " in str(e.value) and "(no CPU path)" in str(e.value)
    assert torch.equal(p, torch.zeros(8))


def vitl_named_parameters():
    from oracle import moge_oracle as O
    spec = O.state_dict_spec(O.named_configs()["moge-2-vitl-normal"])
    return [(name, torch.zeros(1)) for name, _ in spec]          # one element each: only the names matter here


def test_build_optimizer_groups_the_vitl_names_as_the_config_says():
    named = vitl_named_parameters()
    opt = M.build_optimizer(named, BLOCKS["optimizer"], max_grad_norm=1.0, ema_decay=0.999)
    assert isinstance(opt, M.AdamW) and opt.max_grad_norm == 1.0 and len(opt.param_groups) == 2
    assert [g["lr"] for g in opt.param_groups] == [1e-4, 1e-5]
    by_id = {id(p): name for name, p in named}
    slow = sorted(by_id[id(p)] for p in opt.param_groups[1]["params"])
    assert slow == sorted(name for name, _ in named if name.startswith("encoder.backbone.")) and len(slow) > 300
    fast = [by_id[id(p)] for p in opt.param_groups[0]["params"]]
    assert len(fast) + len(slow) == len(named) and not any(".backbone." in name for name in fast)
    assert [by_id[id(p)] for p in opt.param_groups[0]["params"]] == [name for name, _ in named if ".backbone." not in name]          # model order kept
    module = torch.nn.Sequential(torch.nn.Linear(2, 2))
    other = M.build_optimizer(module, {"type": "SGD", "params": [{"params": {"include": ["*"]}, "lr": 0.1}]})
    assert isinstance(other, torch.optim.SGD) and len(other.param_groups[0]["params"]) == 2


def test_build_optimizer_asserts_when_a_trainable_parameter_is_left_out():
    named = [("head.weight", torch.zeros(2, requires_grad=True)), ("encoder.backbone.x", torch.zeros(2, requires_grad=True)), ("frozen", torch.zeros(2))]
    config = {"type": "AdamW", "params": [{"params": {"include": ["head.*"]}, "lr": 1e-4}]}
    with pytest.raises(AssertionError, match="encoder.backbone.x"):
        M.build_optimizer(named, config)
    named[1][1].requires_grad_(False)
    assert len(M.build_optimizer(named, config).param_groups[0]["params"]) == 1          # a frozen one may stay out


def test_build_lr_scheduler_gives_the_lr_sequence_of_torch_adamw():
    import warnings

    def sequence(cls):
        named = [("head.w", torch.zeros(2)), ("encoder.backbone.w", torch.zeros(2))]
        groups = [{"params": [named[0][1]], "lr": 1e-4}, {"params": [named[1][1]], "lr": 1e-5}]
        opt = cls(groups)
        sched = M.build_lr_scheduler(opt, BLOCKS["lr_scheduler"])
        out = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                      # "lr_scheduler.step() before optimizer.step()": no step is taken here
            for _ in range(3000):
                out.append([g["lr"] for g in opt.param_groups])
                sched.step()
        return out

    ours, theirs = sequence(M.AdamW), sequence(torch.optim.AdamW)
    assert ours == theirs
    assert ours[0] == [1e-4, 0.0] and ours[1500] == [1e-4, 0.5e-5] and ours[2999] == [1e-4, 1e-5]
    assert isinstance(M.build_lr_scheduler(M.AdamW([torch.zeros(1)]), {"type": "LambdaLR", "params": {"lr_lambda": "0.5 ** (epoch // 10)"}}),
                      torch.optim.lr_scheduler.LambdaLR)
    assert isinstance(M.build_lr_scheduler(M.AdamW([torch.zeros(1)]), {"type": "ExponentialLR", "params": {"gamma": 0.9}}), torch.optim.lr_scheduler.ExponentialLR)


def test_state_dict_exchanges_with_torch_adamw_in_both_directions():
    ours = M.AdamW(F.param_groups(F.initial()))
    theirs = torch.optim.AdamW(F.param_groups(F.initial()), foreach=False)
    theirs.load_state_dict(ours.state_dict())                    # fresh -> torch
    assert [g["lr"] for g in theirs.param_groups] == [1e-4, 1e-5] and theirs.param_groups[1]["betas"] == (0.8, 0.99) and not theirs.state
    params = [p for g in theirs.param_groups for p in g["params"]]
    for p in params:
        p.grad = torch.ones_like(p)
    theirs.step()                                                # the loaded groups hold every key torch's step needs
    theirs.step()
    ours.load_state_dict(theirs.state_dict())                    # torch -> here
    assert ours._pending_steps == 2.0
    mine = [p for g in ours.param_groups for p in g["params"]]
    for a, b in zip(mine, params):
        assert torch.equal(ours.state[a]["exp_avg"], theirs.state[b]["exp_avg"]) and torch.equal(ours.state[a]["exp_avg_sq"], theirs.state[b]["exp_avg_sq"])
    back = ours.state_dict()
    assert back["state"].keys() == theirs.state_dict()["state"].keys() and float(back["state"][0]["step"]) == 2.0
    with pytest.raises(ValueError, match="amsgrad"):
        bad = theirs.state_dict()
        bad["param_groups"][0]["amsgrad"] = True
        ours.load_state_dict(bad)
