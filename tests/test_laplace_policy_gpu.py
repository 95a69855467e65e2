"""ovla_laplace_sample / ovla_laplace_pg against the numpy contract (tests/laplace_policy_reference.py): bit for bit where every operation is IEEE
(both kernels' log-probabilities, `clipped`, the surrogate gradient given the kernel's own ratio bits, the KL term on policy), within the
reference's derived bounds where logf, expf and expm1f enter, and the identities that tie the two kernels, the group form and the L1 gradient
together.  Shapes: rows 1 / 24 / 67 (one lane, part of a workgroup, more than one workgroup of the sampler), action dimensions on and around
the Philox word boundaries up to the maximum, G = 1 / 2 / the cap."""
import importlib

import numpy as np
import pytest
import torch

from tests import laplace_policy_reference as L

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
ROWS = (1, 24, 67)
ADIMS = (1, 4, 5, 7, 14, 16)
GS = (1, 2, 64)
SEED, CALL = 0x9E3779B97F4A7C15, 41


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def same(a, b, what):
    assert a.shape == b.shape and torch.equal(bits(a), bits(b)), f"{what}: bits differ"


def same_np(got, want32, what):
    got = got.detach().cpu().numpy()
    assert got.shape == want32.shape and np.array_equal(got.view(np.int32), np.asarray(want32, dtype=np.float32).view(np.int32)), f"{what}: bits differ"


def _keys(rows, G):
    """int32 row keys, negative ones among them, all distinct."""
    return (torch.arange(rows * G, dtype=torch.int64).view(rows, G) * 7919 - 300000).to(torch.int32)


def _world(dev, rows, adim, G, seed=0):
    g = torch.Generator().manual_seed(1000 * adim + 10 * G + rows + seed)
    mu = L.means(g, rows, adim)
    return g, mu, torch.from_numpy(mu).to(BF).to(dev), _keys(rows, G)


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("adim", ADIMS)
def test_sample_against_the_reference(ops, dev, adim, G):
    scale = L.SCALES[adim]
    b, inv_b, log_norm = L.scales(scale, adim)
    for rows in ROWS:
        _, mu, pred, keys = _world(dev, rows, adim, G)
        act, lp = ops.laplace_sample(pred, scale, G, seed=SEED, call=CALL, row_key=keys.to(dev))
        assert act.shape == (rows, G, adim) and lp.shape == (rows, G) and act.dtype == F32 and lp.dtype == F32
        ref = L.sample_ref(mu, scale, G, seed=SEED, call=CALL, row_keys=keys.numpy())
        a = act.cpu().numpy()
        err = np.abs(a.astype(np.float64) - ref["action"])
        print(f"rows {rows} adim {adim} G {G}: max action error / bound = {float((err / ref['action_bound']).max()):.3f}")
        assert bool(np.all(err <= ref["action_bound"])), f"rows {rows}: action error {err.max():.3e} beyond the derived bound"
        same_np(lp, L.logprob32(mu, a, inv_b, log_norm), f"rows {rows}: the sampler's logprob from its stored actions")
        # the other kernel reports the same bits for the stored draws
        lp2 = ops.laplace_pg(pred, act, torch.ones((rows, G), dtype=F32, device=dev), scale)[0]
        same(lp2, lp, f"rows {rows}: ovla_laplace_pg's logprob of the sampler's draws")
        # default keys r * G + g
        dflt = ops.laplace_sample(pred, scale, G, seed=SEED, call=CALL)
        expl = ops.laplace_sample(pred, scale, G, seed=SEED, call=CALL, row_key=torch.arange(rows * G, dtype=torch.int32, device=dev).view(rows, G))
        same(dflt[0], expl[0], "default keys: action"), same(dflt[1], expl[1], "default keys: logprob")
        if rows * G * adim >= 64:
            assert not torch.equal(dflt[0], act), "the row keys do not reach the generator"


def _pg_inputs(dev, rows, adim, G, ops):
    g, mu, pred, keys = _world(dev, rows, adim, G, seed=5)
    scale = L.SCALES[adim]
    act, lp = ops.laplace_sample(pred, scale, G, seed=SEED, call=CALL + 1, row_key=keys.to(dev))
    adv = torch.randint(1, 9, (rows, G), generator=g).float() / 4.0 * torch.where(torch.rand((rows, G), generator=g) < 0.5, -1.0, 1.0)
    # ratios e^(+-0.5) and e^(+-0.05): at least 4 % away from the clip bounds 0.8 / 1.2 on either side (the reference asserts 1e-3)
    idx = torch.arange(rows * G).view(rows, G)
    shift = torch.where(idx % 2 == 0, 0.5, -0.05) * torch.where(idx % 3 == 0, -1.0, 1.0)
    old = (lp.cpu() + shift).contiguous()
    # the reference prediction: equal to pred on every third dimension (on policy there), up to +-1/4 off elsewhere
    off = torch.randint(-16, 17, (rows, adim), generator=g).float() / 64.0
    off[:, ::3] = 0.0
    ref_pred = (torch.from_numpy(mu) + off).to(BF)
    return mu, pred, scale, act, lp, adv.to(dev), old.to(dev), ref_pred.to(dev)


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("adim", ADIMS)
def test_pg_against_the_reference(ops, dev, adim, G):
    kw = dict(kl_coef=0.375, clip=(0.8, 1.2), grad_scale=1.0 / 24, kl_scale=1.0 / 3)
    for rows in ROWS:
        mu, pred, scale, act, lp_draw, adv, old, ref_pred = _pg_inputs(dev, rows, adim, G, ops)
        lp, ratio, clipped, kl, dpred = ops.laplace_pg(pred, act, adv, scale, old_logprob=old, ref_pred=ref_pred, **kw)
        lp0, ratio0, clipped0, none, dpred0 = ops.laplace_pg(pred, act, adv, scale, old_logprob=old, clip=kw["clip"], grad_scale=kw["grad_scale"])
        assert none is None and kl.shape == (rows,) and dpred.shape == (rows, adim) and dpred.dtype == BF
        same(lp, lp_draw, f"rows {rows}: logprob of the stored draws"), same(lp0, lp, "logprob without the KL term")
        same(ratio0, ratio, "ratio without the KL term"), same(clipped0, clipped, "clipped without the KL term")
        args = (mu, act.cpu().numpy(), adv.cpu().numpy(), scale)
        ref = L.pg_ref(*args, old_logprob=old.cpu().numpy(), ref_pred=ref_pred.float().cpu().numpy(), ratio_bits=ratio.cpu().numpy(), **kw)
        ref0 = L.pg_ref(*args, old_logprob=old.cpu().numpy(), ratio_bits=ratio.cpu().numpy(), clip=kw["clip"], grad_scale=kw["grad_scale"])
        same_np(lp, ref["logprob"], f"rows {rows}: logprob")
        assert np.array_equal(clipped.cpu().numpy(), ref["clipped"]), f"rows {rows}: clipped"
        if G > 1 and rows > 1:
            assert 0 < int(ref["clipped"].sum()) < rows * G, "the inputs exercise neither side of the gate"
        rerr = np.abs(ratio.cpu().numpy().astype(np.float64) - ref["ratio"])
        assert bool(np.all(rerr <= ref["ratio_bound"])), f"rows {rows}: ratio error {rerr.max():.3e} beyond expf's bound"
        # the surrogate term: bit for bit given the kernel's own ratio bits
        assert np.array_equal(bits(dpred0).numpy().view(np.uint16), ref0["dpred_bits"]), f"rows {rows}: dpred of the surrogate"
        # the KL term
        kerr = np.abs(kl.cpu().numpy().astype(np.float64) - ref["kl"])
        print(f"rows {rows} adim {adim} G {G}: max kl error / bound = {float((kerr / np.maximum(ref['kl_bound'], 1e-300)).max()):.3f}")
        assert bool(np.all(kerr <= ref["kl_bound"])), f"rows {rows}: kl error {kerr.max():.3e} beyond the derived bound"
        got = dpred.float().cpu().numpy()
        assert bool(np.all((got >= ref["dpred_lo"]) & (got <= ref["dpred_hi"]))), f"rows {rows}: dpred with the KL term outside [lo, hi]"
        split = ref["dpred_lo"] != ref["dpred_hi"]
        assert split.mean() < 0.05, "the one-ulp allowance is the exception (a rounding boundary within the bound), not the rule"
        on = ref["kl_on_policy"]
        assert on.any() and (adim == 1 or not on.all())
        # ref_pred == pred: kl and its gradient are exactly +0
        _, _, _, kl_on, dpred_on = ops.laplace_pg(pred, act, adv, scale, old_logprob=old, ref_pred=pred.clone(), **kw)
        assert bool((bits(kl_on) == 0).all()), "kl on policy is not +0"
        want = (dpred0.float() + 0.0).to(BF)                      # (-0 + +0 = +0: the only bits an added +0 can change)
        same(dpred_on, want, f"rows {rows}: dpred on policy")


def test_group_draw_is_the_single_draw_and_rows_are_isolated(ops, dev):
    rows, adim, G = 24, 7, 4
    _, mu, pred, keys = _world(dev, rows, adim, G)
    scale = L.SCALES[adim]
    act, lp = ops.laplace_sample(pred, scale, G, seed=SEED, call=CALL, row_key=keys.to(dev))
    for g in range(G):
        a1, l1 = ops.laplace_sample(pred, scale, 1, seed=SEED, call=CALL, row_key=keys[:, g:g + 1].contiguous().to(dev))
        same(a1[:, 0], act[:, g], f"draw {g}: action"), same(l1[:, 0], lp[:, g], f"draw {g}: logprob")
    assert not torch.equal(act[:, 0], act[:, 1])
    # a row alone, and in another batch at another position, under its own keys
    for r in (0, 5, 23):
        a1, l1 = ops.laplace_sample(pred[r:r + 1].contiguous(), scale, G, seed=SEED, call=CALL, row_key=keys[r:r + 1].contiguous().to(dev))
        same(a1[0], act[r], f"row {r} alone: action"), same(l1[0], lp[r], f"row {r} alone: logprob")
    perm = torch.randperm(rows, generator=torch.Generator().manual_seed(1))
    a2, l2 = ops.laplace_sample(pred[perm.to(dev)].contiguous(), scale, G, seed=SEED, call=CALL, row_key=keys[perm].contiguous().to(dev))
    same(a2, act[perm.to(dev)], "permuted batch: action"), same(l2, lp[perm.to(dev)], "permuted batch: logprob")
    # the next call draws something else
    assert not torch.equal(ops.laplace_sample(pred, scale, G, seed=SEED, call=CALL + 1, row_key=keys.to(dev))[0], act)
    # ovla_laplace_pg: a row's outputs alone and in the batch
    mu, pred, scale, act, _, adv, old, ref_pred = _pg_inputs(dev, rows, adim, G, ops)
    kw = dict(kl_coef=0.375, grad_scale=1.0 / 24, kl_scale=1.0 / 3)
    full = ops.laplace_pg(pred, act, adv, scale, old_logprob=old, ref_pred=ref_pred, **kw)
    for r in (0, 5, 23):
        one = ops.laplace_pg(pred[r:r + 1].contiguous(), act[r:r + 1].contiguous(), adv[r:r + 1].contiguous(), scale, old_logprob=old[r:r + 1].contiguous(),
                             ref_pred=ref_pred[r:r + 1].contiguous(), **kw)
        for name, a, b in zip(("logprob", "ratio", "clipped", "kl", "dpred"), one, full):
            same(a[0], b[r], f"ovla_laplace_pg row {r} alone: {name}")


def test_state_dev_overrides_the_host_words(ops, dev):
    rows, adim, G = 24, 5, 2
    _, mu, pred, keys = _world(dev, rows, adim, G)
    scale = L.SCALES[adim]
    want = ops.laplace_sample(pred, scale, G, seed=SEED, call=CALL, row_key=keys.to(dev))
    state = torch.from_numpy(np.array([SEED & 0xFFFFFFFF, SEED >> 32, CALL], dtype=np.uint32).view(np.int32)).to(dev)
    got = ops.laplace_sample(pred, scale, G, seed=123, call=7, state_dev=state, row_key=keys.to(dev))
    same(got[0], want[0], "state_dev: action"), same(got[1], want[1], "state_dev: logprob")
    other = ops.laplace_sample(pred, scale, G, seed=123, call=7, row_key=keys.to(dev))
    assert not torch.equal(other[0], want[0])


def test_duplicates_padding_and_the_l1_gradient(ops, dev):
    rows, adim = 24, 7
    mu, pred, scale, act, _, adv, old, _ = _pg_inputs(dev, rows, adim, 1, ops)
    gs = 1.0 / 24
    one = ops.laplace_pg(pred, act, adv, scale, old_logprob=old, grad_scale=gs)
    # G = 2 duplicated draws at half the scale: x + x and the halved scale are exact
    two = ops.laplace_pg(pred, act.expand(rows, 2, adim).contiguous(), adv.expand(rows, 2).contiguous(), scale, old_logprob=old.expand(rows, 2).contiguous(),
                         grad_scale=gs / 2)
    same(two[4], one[4], "G = 2 duplicated draws: dpred")
    same(two[0][:, 0], one[0][:, 0], "G = 2 duplicated draws: logprob")
    # zero-advantage draws full of NaN change nothing
    a3 = torch.full((rows, 3, adim), float("nan"), device=dev)
    a3[:, 1] = act[:, 0]
    adv3, old3 = torch.zeros((rows, 3), device=dev), torch.full((rows, 3), float("nan"), device=dev)
    adv3[:, 1], old3[:, 1] = adv[:, 0], old[:, 0]
    three = ops.laplace_pg(pred, a3, adv3, scale, old_logprob=old3, grad_scale=gs)
    same(three[4], one[4], "two NaN padding draws: dpred")
    same(three[0][:, 1], one[0][:, 0], "two NaN padding draws: the live draw's logprob")
    assert bool((three[2][:, [0, 2]] == 0).all())
    assert bool((one[4].float() != 0).any()) and bool(torch.isfinite(one[4].float()).all())
    # every sample skipped: +0
    zero = ops.laplace_pg(pred, a3, torch.zeros((rows, 3), device=dev), scale, old_logprob=old3, grad_scale=gs)
    assert bool((bits(zero[4]) == 0).all()), "a row with every sample skipped is not +0"
    # G = 1, adv = 1, scale = 1, no old log-probabilities: the L1 loss gradient head_out_bwd_kernel forms, bf16(sign(pred - target) * grad_scale)
    g = torch.Generator().manual_seed(3)
    target = (torch.randint(-64, 65, (rows, adim), generator=g).double() / 64.0).to(BF)
    target[::4] = torch.from_numpy(mu).to(BF)[::4]                # pred == target: the gradient is 0 there
    l1 = ops.laplace_pg(pred, target.float().view(rows, 1, adim).to(dev), torch.ones((rows, 1), device=dev), 1.0, grad_scale=gs)
    d = (pred.float().cpu() - target.float()).to(BF).float()      # head_out_bwd_kernel: d = bfround(pred - target); g = d > 0 ? s : (d < 0 ? -s : 0)
    s = torch.tensor(gs, dtype=F32)
    want = torch.where(d > 0, s, torch.where(d < 0, -s, torch.zeros(()))).to(BF)
    same(l1[4], want, "the L1 gradient")
    assert bool((l1[1] == 1.0).all()) and bool((l1[2] == 0).all())
    same_np(l1[0], L.logprob32(mu, target.float().numpy()[:, None, :], *L.scales(1.0, adim)[1:]), "logprob at scale 1")


def test_refusals_leave_the_outputs_untouched(ops, dev):
    lib = importlib.import_module("openvla-oft_amd._lib")
    rows, adim, G = 3, 7, 2
    _, mu, pred, keys = _world(dev, rows, adim, G)
    act = torch.full((rows, G, adim), -77.0, device=dev)
    lp = torch.full((rows, G), -77.0, device=dev)
    with pytest.raises(lib.OvlaError, match="scale"):
        ops.laplace_sample(pred, [0.5] * 6 + [0.0], G, action=act, logprob=lp)
    act65, lp65 = torch.full((rows, 65, adim), -77.0, device=dev), torch.full((rows, 65), -77.0, device=dev)
    with pytest.raises(lib.OvlaError, match="G = 65"):
        ops.laplace_sample(pred, 0.5, 65, action=act65, logprob=lp65)
    adv = torch.ones((rows, G), device=dev)
    outs = dict(logprob=lp.clone(), ratio=lp.clone(), clipped=torch.full((rows, G), -77, dtype=torch.int32, device=dev), dpred=torch.full((rows, adim), -77.0, dtype=BF, device=dev))
    for kw, phrase in ((dict(clip=(1.3, 1.2)), "clip_lo"), (dict(kl_coef=-1.0), "kl_coef"), (dict(clip=(0.8, float("nan"))), "clip_lo")):
        with pytest.raises(lib.OvlaError, match=phrase):
            ops.laplace_pg(pred, act, adv, 0.5, grad_scale=1.0, **kw, **outs)
    with pytest.raises(lib.OvlaError, match="scale"):
        ops.laplace_pg(pred, act, adv, [0.5] * 6 + [float("inf")], grad_scale=1.0, **outs)
    torch.cuda.synchronize()
    assert bool((act == -77).all()) and bool((lp == -77).all()) and bool((act65 == -77).all()) and bool((lp65 == -77).all())
    for name, t in outs.items():
        assert bool((t.float() == -77).all()), f"a refused call wrote {name}"
