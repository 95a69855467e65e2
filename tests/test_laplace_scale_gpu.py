"""ovla_laplace_sample_rows / ovla_laplace_pg_rows against the numpy contract (tests/laplace_scale_reference.py): bit for bit where every operation
is IEEE given the kernel's own inv_b bits (read through the public entry: the reference's probe) and ratio bits, within the reference's derived
bounds where logf, expf and expm1f enter, and bit for bit against the shipped fixed-scale kernels where the log-scale is 0.  Shapes: rows 1 / 24 /
67 (one lane, part of a workgroup, more than one workgroup of the sampler), action dimensions 1 / 7 / 14 / 16, G = 1 / 2 / the cap."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from tests import laplace_policy_reference as L
from tests import laplace_scale_reference as S

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
ROWS = (1, 24, 67)
ADIMS = (1, 7, 14, 16)
GS = (1, 2, 64)
BOUNDS = S.BOUNDS


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == BF else t.view(torch.int32)


def same(a, b, what):
    assert a.shape == b.shape and torch.equal(bits(a), bits(b)), f"{what}: bits differ"


def same_np(got, want32, what):
    got = got.detach().cpu().numpy()
    assert got.shape == want32.shape and np.array_equal(got.view(np.int32), np.asarray(want32, dtype=np.float32).view(np.int32)), f"{what}: bits differ"


def bf(x, dev):
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(BF).to(dev).contiguous()


def dv(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def probe(ops, dev, s_t):
    """The kernel's own inv_b bits of a bf16 log-scale tensor [rows, adim] (S.probe_inv_b: one launch on [rows * adim, 1])."""
    n = s_t.numel()
    mu0, act, adv = S.probe_args(tuple(s_t.shape))
    lp = ops.laplace_pg_rows(bf(mu0, dev), s_t.reshape(n, 1).contiguous(), BOUNDS, dv(act, dev), dv(adv, dev))[0]
    inv_b = S.probe_inv_b(lp.cpu().numpy(), tuple(s_t.shape), BOUNDS)
    twin = S.elem_ref(s_t.float().cpu().numpy(), BOUNDS)["inv_b"]
    assert bool(np.all(np.abs(inv_b.astype(np.float64) - twin) <= 4 * 2.0 ** -23 * twin)), "the probed inv_b is not expf's value within its ulps"
    return inv_b


def _keys(rows, G):
    return (torch.arange(rows * G, dtype=torch.int64).view(rows, G) * 7919 - 300000).to(torch.int32)


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("adim", ADIMS)
def test_sample_rows_against_the_reference(ops, dev, adim, G):
    for rows in ROWS:
        g = torch.Generator().manual_seed(1000 * adim + 10 * G + rows)
        mu = L.means(g, rows, adim)
        s = S.log_scales(g, rows, adim)
        pred, s_t, keys = bf(mu, dev), bf(s, dev), _keys(rows, G)
        inv_b = probe(ops, dev, s_t)
        act, lp, ent = ops.laplace_sample_rows(pred, s_t, BOUNDS, G, seed=S.SEED, call=S.CALL, row_key=keys.to(dev))
        assert act.shape == (rows, G, adim) and lp.shape == (rows, G) and ent.shape == (rows,) and act.dtype == F32 and lp.dtype == F32 and ent.dtype == F32
        ref = S.sample_rows_ref(mu, s, BOUNDS, G, seed=S.SEED, call=S.CALL, row_keys=keys.numpy(), inv_b_bits=inv_b)
        a = act.cpu().numpy()
        err = np.abs(a.astype(np.float64) - ref["action"])
        print(f"rows {rows} adim {adim} G {G}: max action error / bound = {float((err / ref['action_bound']).max()):.3f}")
        assert bool(np.all(err <= ref["action_bound"])), f"rows {rows}: action error {err.max():.3e} beyond the derived bound"
        el = ref["elem"]
        same_np(lp, S.logprob32(mu, a, el["inv_b"], el["log_norm"]), f"rows {rows}: the sampler's logprob from its stored actions")
        same_np(ent, ref["entropy"], f"rows {rows}: entropy")
        out = ops.laplace_pg_rows(pred, s_t, BOUNDS, act, torch.ones((rows, G), dtype=F32, device=dev))
        same(out[0], lp, f"rows {rows}: ovla_laplace_pg_rows' logprob of the sampler's draws"), same(out[4], ent, f"rows {rows}: the two kernels' entropy")
        dflt = ops.laplace_sample_rows(pred, s_t, BOUNDS, G, seed=S.SEED, call=S.CALL)
        expl = ops.laplace_sample_rows(pred, s_t, BOUNDS, G, seed=S.SEED, call=S.CALL, row_key=torch.arange(rows * G, dtype=torch.int32, device=dev).view(rows, G))
        same(dflt[0], expl[0], "default keys: action"), same(dflt[1], expl[1], "default keys: logprob")
        if rows * G * adim >= 64:
            assert not torch.equal(dflt[0], act), "the row keys do not reach the generator"


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("adim", ADIMS)
def test_pg_rows_against_the_reference(ops, dev, adim, G):
    kw = S.PG_KW
    kw0 = dict(clip=kw["clip"], grad_scale=kw["grad_scale"], entropy_coef=kw["entropy_coef"], ent_scale=kw["ent_scale"])
    for rows in ROWS:
        w = S.pg_inputs(rows, adim, G)
        pred, s_t, act, adv, old = bf(w["mu"], dev), bf(w["s"], dev), dv(w["act"], dev), dv(w["adv"], dev), dv(w["old"], dev)
        ref_pred, ref_s = bf(w["ref_mu"], dev), bf(w["ref_s"], dev)
        inv_b = probe(ops, dev, s_t)
        lp, ratio, clipped, kl, ent, dpred, dls = ops.laplace_pg_rows(pred, s_t, BOUNDS, act, adv, old_logprob=old, ref_pred=ref_pred, ref_log_scale=ref_s, **kw)
        lp0, ratio0, clipped0, none, ent0, dpred0, dls0 = ops.laplace_pg_rows(pred, s_t, BOUNDS, act, adv, old_logprob=old, **kw0)
        assert none is None and kl.shape == (rows,) and dpred.shape == (rows, adim) and dls.shape == (rows, adim) and dls.dtype == BF
        same(lp0, lp, "logprob without the KL term"), same(ratio0, ratio, "ratio without the KL term"), same(clipped0, clipped, "clipped without the KL term")
        same(ent0, ent, "entropy without the KL term")
        args = (w["mu"], w["s"], BOUNDS, w["act"], w["adv"])
        rb = dict(ratio_bits=ratio.cpu().numpy(), inv_b_bits=inv_b)
        ref = S.pg_rows_ref(*args, old_logprob=w["old"], ref_pred=w["ref_mu"], ref_log_scale=w["ref_s"], **rb, **kw)
        ref0 = S.pg_rows_ref(*args, old_logprob=w["old"], **rb, **kw0)
        same_np(lp, ref["logprob"], f"rows {rows}: logprob"), same_np(ent, ref["entropy"], f"rows {rows}: entropy")
        assert np.array_equal(clipped.cpu().numpy(), ref["clipped"]), f"rows {rows}: clipped"
        if G > 1 and rows > 1:
            assert 0 < int(ref["clipped"].sum()) < rows * G, "the inputs exercise neither side of the gate"
        rerr = np.abs(ratio.cpu().numpy().astype(np.float64) - ref["ratio"])
        assert bool(np.all(rerr <= ref["ratio_bound"])), f"rows {rows}: ratio error {rerr.max():.3e} beyond expf's bound"
        # the surrogate (and the entropy's term): bit for bit given the kernel's own ratio and inv_b bits
        assert np.array_equal(bits(dpred0).numpy().view(np.uint16), ref0["dpred_bits"]), f"rows {rows}: dpred of the surrogate"
        assert np.array_equal(bits(dls0).numpy().view(np.uint16), ref0["dlog_scale_bits"]), f"rows {rows}: dlog_scale of the surrogate and the entropy"
        # the KL term
        kerr = np.abs(kl.cpu().numpy().astype(np.float64) - ref["kl"])
        print(f"rows {rows} adim {adim} G {G}: max kl error / bound = {float((kerr / np.maximum(ref['kl_bound'], 1e-300)).max()):.3f}")
        assert bool(np.all(kerr <= ref["kl_bound"])), f"rows {rows}: kl error {kerr.max():.3e} beyond the derived bound"
        for name, got_t in (("dpred", dpred), ("dlog_scale", dls)):
            got = got_t.float().cpu().numpy()
            lo, hi = ref[name + "_lo"], ref[name + "_hi"]
            assert bool(np.all((got >= lo) & (got <= hi))), f"rows {rows}: {name} with the KL term outside [lo, hi]"
            print(f"rows {rows} adim {adim} G {G}: {name} split on {(lo != hi).mean():.4f} of the elements")
            assert (lo != hi).mean() < 0.05, "the one-ulp allowance is the exception (a rounding boundary within the bound), not the rule"
        with np.errstate(invalid="ignore"):
            out = np.isnan(w["s"]) | (w["s"] < BOUNDS[0]) | (w["s"] > BOUNDS[1])
        if rows * adim >= 7:
            assert int(out.sum()) == 3
        assert bool((bits(dls).numpy()[out] == 0).all()) and bool((bits(dls0).numpy()[out] == 0).all()), "a clamped or NaN log-scale took a gradient"
        for t in (lp, ratio, kl, ent, dpred.float(), dls.float()):
            assert bool(torch.isfinite(t).all())
        on = ref["kl_on_policy"]
        assert on.any() and (adim == 1 or not on.all())
        # the reference is the policy: kl and both of its gradients are exactly +0
        _, _, _, kl_on, _, dpred_on, dls_on = ops.laplace_pg_rows(pred, s_t, BOUNDS, act, adv, old_logprob=old, ref_pred=pred.clone(), ref_log_scale=s_t.clone(), **kw)
        assert bool((bits(kl_on) == 0).all()), "kl on policy is not +0"
        same(dpred_on, (dpred0.float() + 0.0).to(BF), f"rows {rows}: dpred on policy")       # (-0 + +0 = +0: the only bits an added +0 can change)
        on_ref = S.pg_rows_ref(*args, old_logprob=w["old"], ref_pred=w["mu"], ref_log_scale=w["s"], **rb, **kw)
        assert np.array_equal(on_ref["dlog_scale_lo"], on_ref["dlog_scale_hi"])
        assert np.array_equal(dls_on.float().cpu().numpy().view(np.int32), on_ref["dlog_scale_lo"].view(np.int32)), f"rows {rows}: dlog_scale on policy"


@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("adim", ADIMS)
def test_zero_log_scale_is_the_fixed_scale_kernels_at_one(ops, dev, adim, G):
    kw = dict(kl_coef=0.375, clip=(0.8, 1.2), grad_scale=1.0 / 24, kl_scale=1.0 / 3)
    for rows in ROWS:
        w = S.pg_inputs(rows, adim, G, seed=9)
        pred, keys, zero = bf(w["mu"], dev), _keys(rows, G).to(dev), torch.zeros((rows, adim), dtype=BF, device=dev)
        a1, l1 = ops.laplace_sample(pred, 1.0, G, seed=S.SEED, call=S.CALL, row_key=keys)
        a2, l2, _ = ops.laplace_sample_rows(pred, zero, BOUNDS, G, seed=S.SEED, call=S.CALL, row_key=keys)
        same(a2, a1, f"rows {rows}: action"), same(l2, l1, f"rows {rows}: logprob")
        adv, ref_pred = dv(w["adv"], dev), bf(w["ref_mu"], dev)
        idx = torch.arange(rows * G).view(rows, G)
        old = (l1.cpu() + torch.where(idx % 2 == 0, 0.5, -0.05) * torch.where(idx % 3 == 0, -1.0, 1.0)).contiguous().to(dev)
        want = ops.laplace_pg(pred, a1, adv, 1.0, old_logprob=old, ref_pred=ref_pred, **kw)
        got = ops.laplace_pg_rows(pred, zero, BOUNDS, a1, adv, old_logprob=old, ref_pred=ref_pred, ref_log_scale=zero.clone(), want_dlog_scale=False, **kw)
        assert got[6] is None
        for name, i, j in (("logprob", 0, 0), ("ratio", 1, 1), ("clipped", 2, 2), ("kl", 3, 3), ("dpred", 5, 4)):
            same(got[i], want[j], f"rows {rows}: {name}")
        if rows > 1 and adim > 1:                                    # (dimension 0 is on policy by construction)
            assert bool((want[3] > 0).any()), "the anchor's KL term is empty"


def test_rows_are_isolated_and_a_skipped_nan_draw_changes_nothing(ops, dev):
    rows, adim, G = 24, 7, 4
    w = S.pg_inputs(rows, adim, G)
    pred, s_t, act, adv, old = bf(w["mu"], dev), bf(w["s"], dev), dv(w["act"], dev), dv(w["adv"], dev), dv(w["old"], dev)
    ref_pred, ref_s, keys = bf(w["ref_mu"], dev), bf(w["ref_s"], dev), _keys(rows, G)
    names = ("logprob", "ratio", "clipped", "kl", "entropy", "dpred", "dlog_scale")
    full = ops.laplace_pg_rows(pred, s_t, BOUNDS, act, adv, old_logprob=old, ref_pred=ref_pred, ref_log_scale=ref_s, **S.PG_KW)
    smp = ops.laplace_sample_rows(pred, s_t, BOUNDS, G, seed=S.SEED, call=S.CALL, row_key=keys.to(dev))
    for r in (0, 5, 23):
        sl = lambda t: t[r:r + 1].contiguous()
        one = ops.laplace_pg_rows(sl(pred), sl(s_t), BOUNDS, sl(act), sl(adv), old_logprob=sl(old), ref_pred=sl(ref_pred), ref_log_scale=sl(ref_s), **S.PG_KW)
        for name, a, b in zip(names, one, full):
            same(a[0], b[r], f"ovla_laplace_pg_rows row {r} alone: {name}")
        s1 = ops.laplace_sample_rows(sl(pred), sl(s_t), BOUNDS, G, seed=S.SEED, call=S.CALL, row_key=sl(keys).to(dev))
        for name, a, b in zip(("action", "logprob", "entropy"), s1, smp):
            same(a[0], b[r], f"ovla_laplace_sample_rows row {r} alone: {name}")
    # two zero-advantage draws full of NaN around the live ones: nothing changes and the row stays finite
    a6 = torch.full((rows, G + 2, adim), float("nan"), device=dev)
    adv6, old6 = torch.zeros((rows, G + 2), device=dev), torch.full((rows, G + 2), float("nan"), device=dev)
    a6[:, 1:G + 1], adv6[:, 1:G + 1], old6[:, 1:G + 1] = act, adv, old
    kw = dict(S.PG_KW, grad_scale=S.PG_KW["grad_scale"])
    pad = ops.laplace_pg_rows(pred, s_t, BOUNDS, a6, adv6, old_logprob=old6, ref_pred=ref_pred, ref_log_scale=ref_s, **kw)
    same(pad[5], full[5], "NaN padding draws: dpred"), same(pad[6], full[6], "NaN padding draws: dlog_scale")
    same(pad[0][:, 1:G + 1].contiguous(), full[0], "NaN padding draws: the live draws' logprob")
    assert bool((pad[2][:, [0, G + 1]] == 0).all()) and bool(torch.isfinite(pad[5].float()).all()) and bool(torch.isfinite(pad[6].float()).all())
    # every sample skipped, no reference, no entropy bonus: both gradients are +0
    zero = ops.laplace_pg_rows(pred, s_t, BOUNDS, a6, torch.zeros((rows, G + 2), device=dev), old_logprob=old6, grad_scale=1.0)
    assert bool((bits(zero[5]) == 0).all()) and bool((bits(zero[6]) == 0).all()), "a row with every sample skipped is not +0"
    # G = 1, adv = 1, no ratio, no reference, no entropy: the gradient of the Laplace negative log-likelihood of a target chunk
    inv_b = probe(ops, dev, s_t)
    tgt = L.bf16_round((w["mu"] + np.where(np.arange(adim) % 2 == 0, 0.25, -0.5).astype(np.float32)).astype(np.float32))
    gs = 1.0 / 24
    nll = ops.laplace_pg_rows(pred, s_t, BOUNDS, dv(tgt[:, None, :], dev), torch.ones((rows, 1), device=dev), grad_scale=gs)
    el = S.elem_ref(w["s"], BOUNDS, inv_b)
    q = (np.abs((tgt - w["mu"]).astype(np.float32)) * el["inv_b"]).astype(np.float32)
    want = np.where(el["inside"], L.bf16_round(((np.float32(1.0) - q).astype(np.float32) * np.float32(gs)).astype(np.float32)), np.float32(0.0))
    assert np.array_equal(nll[6].float().cpu().numpy().view(np.int32), want.astype(np.float32).view(np.int32)), "dlog_scale of the NLL"
    assert bool((nll[1] == 1.0).all()) and bool((nll[2] == 0).all())


def test_refusals_leave_the_outputs_untouched(ops, dev):
    lib = importlib.import_module("openvla-oft_amd._lib")
    rows, adim, G = 3, 7, 2
    w = S.pg_inputs(rows, adim, G)
    pred, s_t, act_in, adv = bf(w["mu"], dev), bf(w["s"], dev), dv(w["act"], dev), dv(w["adv"], dev)
    act = torch.full((rows, G, adim), -77.0, device=dev)
    lp = torch.full((rows, G), -77.0, device=dev)
    ent = torch.full((rows,), -77.0, device=dev)
    souts = dict(action=act, logprob=lp, entropy=ent)
    for b, phrase in (((1.0, -6.0), "bounds"), ((float("-inf"), 1.0), "bounds"), ((-6.0, float("nan")), "bounds"), ((-6.0, float("inf")), "bounds")):
        with pytest.raises(lib.OvlaError, match=phrase):
            ops.laplace_sample_rows(pred, s_t, b, G, **souts)
    act65, lp65 = torch.full((rows, 65, adim), -77.0, device=dev), torch.full((rows, 65), -77.0, device=dev)
    with pytest.raises(lib.OvlaError, match="G = 65"):
        ops.laplace_sample_rows(pred, s_t, BOUNDS, 65, action=act65, logprob=lp65, entropy=ent)
    outs = dict(logprob=lp.clone(), ratio=lp.clone(), clipped=torch.full((rows, G), -77, dtype=torch.int32, device=dev), entropy=ent.clone(),
                dpred=torch.full((rows, adim), -77.0, dtype=BF, device=dev), dlog_scale=torch.full((rows, adim), -77.0, dtype=BF, device=dev))
    klt = torch.full((rows,), -77.0, device=dev)
    for kw, phrase in ((dict(clip=(1.3, 1.2)), "clip_lo"), (dict(kl_coef=-1.0), "kl_coef"), (dict(clip=(0.8, float("nan"))), "clip_lo"),
                       (dict(entropy_coef=-0.5), "entropy_coef"), (dict(entropy_coef=float("nan")), "entropy_coef"),
                       (dict(ref_pred=pred.clone(), kl=klt), "come together"), (dict(ref_log_scale=s_t.clone()), "come together"),
                       (dict(ref_pred=pred.clone(), ref_log_scale=s_t.clone(), kl_coef=float("nan"), kl=klt), "kl_coef")):
        with pytest.raises(lib.OvlaError, match=phrase):
            ops.laplace_pg_rows(pred, s_t, BOUNDS, act_in, adv, grad_scale=1.0, **kw, **outs)
    for b in ((1.0, -6.0), (float("nan"), 1.0), (-6.0, float("inf"))):
        with pytest.raises(lib.OvlaError, match="bounds"):
            ops.laplace_pg_rows(pred, s_t, b, act_in, adv, grad_scale=1.0, **outs)
    # a null log_scale cannot be passed through the wrapper: the entry itself
    g = lib.STRUCTS["ovla_laplace_pg_rows_args"]()
    g.pred, g.log_scale, g.actions, g.advantage = pred.data_ptr(), None, act_in.data_ptr(), adv.data_ptr()
    g.logprob, g.ratio, g.clipped, g.entropy = outs["logprob"].data_ptr(), outs["ratio"].data_ptr(), outs["clipped"].data_ptr(), outs["entropy"].data_ptr()
    g.s_lo, g.s_hi, g.clip_lo, g.clip_hi, g.rows, g.adim, g.G = BOUNDS[0], BOUNDS[1], 0.8, 1.2, rows, adim, G
    assert lib.lib().ovla_laplace_pg_rows(ctypes.byref(g), None) == -1 and b"null pointer" in lib.lib().ovla_last_error()
    torch.cuda.synchronize()
    assert bool((act == -77).all()) and bool((lp == -77).all()) and bool((ent == -77).all()) and bool((act65 == -77).all()) and bool((lp65 == -77).all())
    assert bool((klt == -77).all())
    for name, t in outs.items():
        assert bool((t.float() == -77).all()), f"a refused call wrote {name}"
