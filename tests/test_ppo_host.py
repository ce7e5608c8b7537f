"""CPU tests (-m "not gpu") of the host code the solo and the population PPO paths share (ppo.minibatch_buffers /
minibatch_schedule, policy.kernel_layout, ppo.hyper_row, the updaters' Acas2dPpoUpdateSet): nothing is launched."""
import dataclasses

import pytest
import torch


@pytest.fixture(scope="module")
def g():
    import gym_acas2d_amd as g
    return g


def _run_schedule(g, n, batch_size, lead=()):
    """The schedule of one epoch over a fixed permutation: (rows, mb_idx, mb_tail, [(yielded object, its rows then)])."""
    gen = torch.Generator().manual_seed(n)
    rows = torch.stack([torch.randperm(n, generator=gen) for _ in range(lead[0])]) if lead else torch.randperm(n, generator=gen)
    mb_idx, mb_tail = g.ppo.minibatch_buffers(n, batch_size, "cpu", lead=lead)
    return rows, mb_idx, mb_tail, [(idx, idx.clone()) for idx in g.ppo.minibatch_schedule(rows, mb_idx, mb_tail)]


@pytest.mark.parametrize("lead", [(), (2,)])
def test_schedule_whole_minibatches_then_the_tail(g, lead):
    """n = 10, B = 4: rows 0:4 and 4:8 through mb_idx, then 8:10 through mb_tail -- the buffers themselves are yielded."""
    rows, mb_idx, mb_tail, got = _run_schedule(g, 10, 4, lead)
    assert tuple(mb_idx.shape) == lead + (4,) and tuple(mb_tail.shape) == lead + (2,)
    assert mb_idx.dtype == mb_tail.dtype == torch.int64
    assert [o is b for (o, _), b in zip(got, (mb_idx, mb_idx, mb_tail))] == [True] * 3 and len(got) == 3
    for (_, held), want in zip(got, (rows[..., 0:4], rows[..., 4:8], rows[..., 8:10])):
        assert torch.equal(held, want)


def test_schedule_drops_a_one_row_tail(g):
    """n = 9, B = 4: the ninth row alone has no standard deviation -- no tail buffer, the row is not taken."""
    rows, mb_idx, mb_tail, got = _run_schedule(g, 9, 4)
    assert mb_tail is None and len(got) == 2 and all(o is mb_idx for o, _ in got)
    assert torch.equal(got[0][1], rows[0:4]) and torch.equal(got[1][1], rows[4:8])


def test_schedule_batch_larger_than_the_buffer(g):
    """n = 3, B = 8: B becomes 3, one minibatch of everything, no tail."""
    rows, mb_idx, mb_tail, got = _run_schedule(g, 3, 8)
    assert mb_idx.shape == (3,) and mb_tail is None and len(got) == 1 and got[0][0] is mb_idx
    assert torch.equal(got[0][1], rows)


def _nets(pol):
    """An ActorCritic's actor and critic as (w1, b1, w2, b2, w3, b3) in torch's layout."""
    pn, vn = pol.mlp_extractor.policy_net, pol.mlp_extractor.value_net
    return ((pn[0].weight, pn[0].bias, pn[2].weight, pn[2].bias, pol.action_net.weight, pol.action_net.bias),
            (vn[0].weight, vn[0].bias, vn[2].weight, vn[2].bias, pol.value_net.weight, pol.value_net.bias))


def _written_out(w1, b1, w2, b2, w3, b3):
    """The kernels' layout of one net as ACAS2DVecEnv.collect always formed it."""
    f32 = lambda t: t.detach().to(torch.float32)  # noqa: E731
    return [f32(w1).t().contiguous(), f32(b1).contiguous(), f32(w2).t().contiguous(), f32(b2).contiguous(),
            f32(w3).reshape(-1).contiguous(), f32(b3).reshape(-1).contiguous()]


@pytest.mark.parametrize("D", [8, 53])
def test_kernel_layout_equals_the_written_out_transposes(g, D):
    torch.manual_seed(D)
    pols = [g.ActorCritic(D) for _ in range(3)]
    with torch.no_grad():
        for pol in pols:                                   # biases and log_std are zero at construction
            for p in pol.parameters():
                p.add_(0.1 * torch.randn_like(p))
    for net in _nets(pols[0]):
        got, want = g.policy.kernel_layout(*net), _written_out(*net)
        assert [tuple(t.shape) for t in got] == [(D, 64), (64,), (64, 64), (64,), (64,), (1,)]
        assert all(torch.equal(a, b) and a.is_contiguous() and a.dtype == torch.float32 for a, b in zip(got, want))
    pset = g.ActorCriticSet.from_members(pols)
    stacks = pset.collector_weights()
    assert len(stacks) == 13 and torch.equal(stacks[12], torch.cat([pol.log_std.detach() for pol in pols]))
    for which, names in enumerate((g.ppo.PARAM_NAMES[:6], g.ppo.PARAM_NAMES[6:12])):
        got = g.policy.kernel_layout(*(pset.params[n] for n in names))
        want = [torch.stack(ts) for ts in zip(*(_written_out(*_nets(pol)[which]) for pol in pols))]
        assert [tuple(t.shape) for t in got] == [(3, D, 64), (3, 64), (3, 64, 64), (3, 64), (3, 64), (3, 1)]
        assert all(torch.equal(a, b) and a.is_contiguous() for a, b in zip(got, want))
        assert all(torch.equal(a, b) for a, b in zip(stacks[6 * which:6 * which + 6], want))


def test_hyper_row_is_the_config_in_slot_order(g):
    cfg = g.PPOConfig(n_steps=7, batch_size=5, n_epochs=3, gamma=0.9, gae_lambda=0.8, clip_range=0.11, learning_rate=1.3e-3,
                      ent_coef=0.017, vf_coef=0.71, max_grad_norm=0.37, seed=99, target_kl=0.02)
    default = g.PPOConfig()
    assert all(getattr(cfg, f.name) != getattr(default, f.name) for f in dataclasses.fields(cfg))
    want = {"clip_range": 0.11, "vf_coef": 0.71, "ent_coef": 0.017, "max_grad_norm": 0.37, "learning_rate": 1.3e-3,
            "beta1": 0.8, "beta2": 0.95, "adam_eps": 1e-7}
    assert g.ppo.hyper_row(cfg, 0.8, 0.95, 1e-7) == [want[s] for s in g.ppo.HYPER_SLOTS] and len(g.ppo.HYPER_SLOTS) == 8
    assert g.ppo.hyper_row(cfg)[5:] == [0.9, 0.999, 1e-5]                     # torch.optim.Adam's betas, SB3's eps


@pytest.mark.parametrize("D", [8, 53])
def test_guarded_solo_update_builds_the_struct_of_a_set_of_one(g, D):
    """FusedUpdate(diagnostics=True) and FusedUpdateSet of K = 1 over the same tensors: the same Acas2dPpoUpdateSet, field
    by field, for the same idx."""
    n, B = 12, 5
    pol, cfg = g.ActorCritic(D), g.PPOConfig(clip_range=0.1, learning_rate=1e-3)
    rollout = [torch.zeros(n, D)] + [torch.zeros(n) for _ in range(4)]
    solo = g.FusedUpdate(pol, cfg, *rollout, diagnostics=True)
    pset = g.ActorCriticSet(1, D)
    pset.params = {name: pol.get_parameter(name).detach().unsqueeze(0) for name in g.ppo.PARAM_NAMES}     # views: the same storage
    many = g.FusedUpdateSet(pset, [cfg], *rollout, diagnostics=True)
    assert solo.guarded and many.guarded and torch.equal(solo.hyper, many.hyper) and solo.hyper.shape == (1, 8)
    assert solo.grad.shape == many.grad.shape[1:] and solo.stats.shape == (8,) and many.stats.shape == (1, 8)
    assert solo.step_count.shape == many.step_count.shape == (1,)
    for name in ("grad", "m", "v", "step_count", "stats", "hyper"):           # the workspace is each updater's own: share it
        setattr(many, name, getattr(solo, name))
    idx = torch.arange(B, dtype=torch.int64)
    a, b = solo._set_struct(idx, 1, B), many._set_struct(idx.unsqueeze(0), 1, B)
    assert type(a) is type(b) is g.native.CPpoUpdateSet
    for name, _ in g.native.CPpoUpdateSet._fields_:
        assert getattr(a, name) == getattr(b, name), name
    assert (a.n_members, a.n_rows, a.obs_dim, a.idx) == (1, B, D, idx.data_ptr())
