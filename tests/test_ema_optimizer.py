"""HipAdamW(ema_decay=...) on a two-Block VIT (embed_dim 64, 32 x 32, patch 8) in fp32 and bf16: the average against the float64 recurrence
over the recorded parameter trajectory (bound: ddim_ref.ema_trajectory64, the per-step bound of tests/test_ema_ops.py carried through the
recurrence), the flat and the per-parameter path, a skipped step under the loss scaler, ema_weights(), ema_state_dict / load_ema_state_dict,
and that nothing changes without ema_decay."""
import copy

import numpy as np
import pytest
import torch

import ddim_ref as R
from det_weights import det_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda"
VARS = ["red", "green", "blue"]
VIT_KW = dict(img_size=[32, 32], patch_size=8, in_chans=3, num_classes=5, embed_dim=64, depth=2, num_heads=2)
DTYPES = [torch.float32, torch.bfloat16]
DECAY = 0.9


def build(dtype, seed=31):
    from UCF_VIT.simple.arch import VIT
    m = VIT(**VIT_KW)
    m.load_state_dict(det_state_dict(m, seed))
    m = m.to(DEV)
    m.set_compute_dtype(dtype)
    return m


def optimizer(m, ema_decay=DECAY):
    from UCF_VIT.utils.misc import configure_optimizer
    return configure_optimizer(m, 1e-3, 0.9, 0.95, 1e-2, ema_decay=ema_decay)


def batches(n):
    g = torch.Generator().manual_seed(5)
    return [(torch.randn(4, 3, 32, 32, generator=g).to(DEV), torch.randint(0, 5, (4,), generator=g).to(DEV)) for _ in range(n)]


def backward(m, batch):
    from UCF_VIT.utils.metrics import cross_entropy_loss
    loss = cross_entropy_loss(m(batch[0], VARS), batch[1])
    loss.backward()
    return loss


def snapshot(m):
    return {k: p.detach().cpu().numpy().copy() for k, p in m.named_parameters()}


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def train(m, opt, data):
    traj = [snapshot(m)]
    for b in data:
        backward(m, b)
        opt.step()
        opt.zero_grad()
        traj.append(snapshot(m))
    return traj


@pytest.mark.parametrize("dtype", DTYPES)
def test_average_follows_the_float64_recurrence(dtype):
    m = build(dtype)
    opt = optimizer(m)
    sd0 = opt.ema_state_dict(m)
    assert all(same_bits(sd0[k], v) for k, v in m.state_dict().items())            # before the first step: the parameters themselves
    traj = train(m, opt, batches(3))
    assert bool(opt._ema_flat), "the flat one-launch path was not taken"
    ema = opt.ema_state_dict(m)
    worst = 0.0
    for k, _ in m.named_parameters():
        want, bound = R.ema_trajectory64([t[k] for t in traj], 1.0 - DECAY)
        err = np.abs(ema[k].cpu().numpy().astype(np.float64) - want)
        worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
        assert (err <= bound).all(), k
        assert not np.array_equal(traj[0][k], traj[-1][k]), k
        assert not same_bits(ema[k], m.state_dict()[k]), k                         # an average, not the last iterate
    print(f"{dtype}: worst ema err / bound after 3 steps {worst:.3f}")
    # the optimizer's own state_dict keeps torch.optim.AdamW's layout
    sd = opt.state_dict()
    assert set(sd["state"].keys()) == set(range(len(list(m.parameters()))))
    assert all(set(e.keys()) == {"step", "exp_avg", "exp_avg_sq"} for e in sd["state"].values())
    assert all("ema" not in k for g in sd["param_groups"] for k in g)


@pytest.mark.parametrize("dtype", DTYPES)
def test_flat_and_per_parameter_path_give_the_same_bits(dtype):
    """one step from equal weights and equal gradients.  In the second model one gradient of the weight-decayed group is taken away before
    the step, so that group leaves the flat path (every parameter of a flat run needs its gradient in the flat buffer) and is updated
    parameter by parameter; the parameter without a gradient does not move and its average is the parameter."""
    data = batches(1)
    ma, mb = build(dtype), build(dtype)
    oa, ob = optimizer(ma), optimizer(mb)
    backward(ma, data[0]), backward(mb, data[0])
    left_out = "head.bias"
    dict(mb.named_parameters())[left_out].grad = None
    p_before = dict(mb.named_parameters())[left_out].detach().clone()
    calls = []
    from UCF_VIT._hip import ops
    real = ops.adamw_ema

    def spy(p, *a, **k):
        calls.append(p.numel())
        return real(p, *a, **k)

    ops.adamw_ema = spy
    try:
        oa.step()
        na = len(calls)
        ob.step()
    finally:
        ops.adamw_ema = real
    n_params = len(list(mb.parameters()))
    assert na == 2 and len(calls) - na > 2                                          # two flat runs; then one launch per parameter
    ea, eb = oa.ema_state_dict(ma), ob.ema_state_dict(mb)
    for k, p in mb.named_parameters():
        if k == left_out:
            assert same_bits(p, p_before) and same_bits(eb[k], p_before)
        else:
            assert same_bits(eb[k], ea[k]), k
            assert same_bits(p, dict(ma.named_parameters())[k]), k
    assert len(calls) - na <= n_params


def test_a_skipped_step_leaves_the_average_alone():
    from UCF_VIT.utils.misc import configure_grad_scaler
    m = build(torch.bfloat16)
    opt = optimizer(m)
    sc = configure_grad_scaler(True)
    data = batches(3)
    emas = []
    for i, b in enumerate(data):
        if i == 1:
            b = (b[0].clone(), b[1])
            b[0][0] = float("inf")                                                 # one image of Inf: non-finite gradients
        backward_scaled(m, b, sc)
        before = m._ucf_store.flat_p.clone()
        sc.step(opt)
        sc.update()
        opt.zero_grad()
        emas.append({k: v.clone() for k, v in opt.ema_state_dict(m).items()})
        moved = not same_bits(before, m._ucf_store.flat_p)
        assert moved == (i != 1)
    assert sc.counters() == (2, 1)
    keys = [k for k, _ in m.named_parameters()]
    assert all(same_bits(emas[1][k], emas[0][k]) for k in keys)                    # the skipped step
    assert all(not same_bits(emas[2][k], emas[1][k]) for k in keys)


def backward_scaled(m, batch, sc):
    from UCF_VIT.utils.metrics import cross_entropy_loss
    loss = cross_entropy_loss(m(batch[0], VARS), batch[1])
    sc.scale(loss).backward()
    return loss


@pytest.mark.parametrize("dtype", DTYPES)
def test_ema_weights_swaps_in_place_and_back(dtype):
    m = build(dtype)
    opt = optimizer(m)
    data = batches(3)
    train(m, opt, data)
    x = data[0][0]
    raw = {k: p.detach().clone() for k, p in m.named_parameters()}
    ema_sd = opt.ema_state_dict(m)
    m.eval()
    with torch.no_grad():
        y_raw = m(x, VARS).float().clone()
        with opt.ema_weights():
            for k, p in m.named_parameters():
                assert same_bits(p, ema_sd[k]), k                                   # the averaged weights sit in the parameters
            y_in = m(x, VARS).float().clone()
        y_back = m(x, VARS).float().clone()
    for k, p in m.named_parameters():
        assert same_bits(p, raw[k]), k
    assert all(same_bits(v, ema_sd[k]) for k, v in opt.ema_state_dict(m).items())
    m2 = build(dtype, seed=77)
    m2.load_state_dict(ema_sd, strict=True)
    m2.eval()
    with torch.no_grad():
        y_ema = m2(x, VARS).float()
    assert same_bits(y_in, y_ema) and same_bits(y_back, y_raw) and not same_bits(y_in, y_raw)
    # the context also restores when its body raises
    with pytest.raises(ZeroDivisionError):
        with opt.ema_weights():
            1 / 0
    assert all(same_bits(p, raw[k]) for k, p in m.named_parameters())
    # training goes on from the raw iterate with the fused path
    m.train()
    train(m, opt, data[:1])
    assert len(opt._ema_flat) == 2


@pytest.mark.parametrize("dtype", DTYPES)
def test_ema_state_dict_round_trip_and_aliases(dtype):
    m = build(dtype)
    opt = optimizer(m)
    data = batches(2)
    train(m, opt, data)
    sd = opt.ema_state_dict(m)
    assert list(sd.keys()) == list(m.state_dict().keys())
    assert "token_embeds.proj.weight" in sd and same_bits(sd["token_embeds.proj.weight"], sd["patch_embed.proj.weight"])
    assert not same_bits(sd["token_embeds.proj.weight"], m.state_dict()["token_embeds.proj.weight"])
    m2 = build(dtype, seed=77)
    m2.load_state_dict(sd, strict=True)
    # a fresh optimizer takes the average back, bit for bit, before and after its first flat step adopts it
    m3 = build(dtype)
    m3.load_state_dict(m.state_dict())
    o3 = optimizer(m3)
    o3.load_state_dict(copy.deepcopy(opt.state_dict()))
    o3.load_ema_state_dict(m3, sd)
    back = o3.ema_state_dict(m3)
    assert all(same_bits(back[k], sd[k]) for k in sd)
    train(m, opt, data[:1])
    train(m3, o3, data[:1])
    assert bool(o3._ema_flat)
    a, b = opt.ema_state_dict(m), o3.ema_state_dict(m3)
    assert all(same_bits(a[k], b[k]) for k in a)                                   # the resumed run continues the same average
    with pytest.raises(KeyError):
        o3.load_ema_state_dict(m3, {k: v for k, v in sd.items() if k != "head.bias"})


@pytest.mark.parametrize("dtype", DTYPES)
def test_without_ema_decay_nothing_changes(dtype):
    from UCF_VIT._hip import ops
    from UCF_VIT.utils.misc import configure_grad_scaler
    names = [n for n in dir(ops) if n.startswith("adamw")]
    assert set(names) == {"adamw", "adamw_ema", "adamw_scaled", "adamw_scaled_ema"}
    calls = []
    real = {n: getattr(ops, n) for n in names}

    def wrap(n):
        def f(*a, **k):
            calls.append(n)
            return real[n](*a, **k)
        return f

    for n in names:
        setattr(ops, n, wrap(n))
    try:
        m = build(dtype)
        opt = optimizer(m, ema_decay=None)
        train(m, opt, batches(2))
        assert calls == ["adamw"] * 4                                              # two groups, two steps, one launch each
        sd = opt.state_dict()
        assert all(set(e.keys()) == {"step", "exp_avg", "exp_avg_sq"} for e in sd["state"].values())
        assert opt._ema == {} and opt._ema_flat == {}
        assert all(same_bits(v, m.state_dict()[k]) for k, v in opt.ema_state_dict(m).items())
        with opt.ema_weights():                                                     # nothing to swap
            pass
        del calls[:]
        sc = configure_grad_scaler(True)
        backward_scaled(m, batches(1)[0], sc)
        sc.step(opt)
        sc.update()
        assert calls == ["adamw_scaled"] * 2
        del calls[:]
        m2 = build(dtype)
        o2 = optimizer(m2)
        train(m2, o2, batches(1))
        backward_scaled(m2, batches(1)[0], sc)
        sc.step(o2)
        assert calls == ["adamw_ema"] * 2 + ["adamw_scaled_ema"] * 2
    finally:
        for n in names:
            setattr(ops, n, real[n])
