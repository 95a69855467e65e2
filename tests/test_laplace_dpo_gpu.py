"""ovla_laplace_dpo through ops.laplace_dpo: its log-probabilities and its gradient bit for bit against the shipped kernels ovla_laplace_pg /
ovla_laplace_pg_rows, h and the margin bit for bit against the numpy twin (tests/laplace_dpo_reference.py) given those log-probabilities, loss and
coef within the twin's derived bounds (bit for bit for IPO), position independence, skipped observations and every refusal.  Shapes (B, chunk,
adim): a workgroup partly filled, a chunk that is no multiple of anything with more than one gradient pass per lane, the smallest launch, and both caps."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from tests import laplace_dpo_reference as D
from tests import laplace_policy_reference as L
from tests import laplace_scale_reference as S

pytestmark = pytest.mark.gpu
BF, F32 = torch.bfloat16, torch.float32
SHAPES = ((3, 8, 7), (2, 25, 14), (1, 1, 1), (2, 64, 16))
BOUNDS = S.BOUNDS
VARIANTS = tuple((lt, nll) for lt in ("sigmoid", "ipo") for nll in (0.0, 0.5))


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


def beta_of(chunk, adim):
    """A margin is a sum over chunk * adim elements of order one: this keeps most z = beta m where the sigmoid is not saturated."""
    return 0.5 / float(np.sqrt(chunk * adim))


def device_inputs(w, dev, learned, adim):
    t = dict(pred=bf(w["mu"], dev), ref_pred=bf(w["ref_mu"], dev), chosen=dv(w["chosen"], dev), rejected=dv(w["rejected"], dev), weight=dv(w["weight"], dev))
    if learned:
        t.update(log_scale=bf(w["s"], dev), ref_log_scale=bf(w["ref_s"], dev))
    return t


def launch(ops, t, chunk, learned, adim, *, weight=True, **kw):
    scale = dict(log_scale=t["log_scale"], ref_log_scale=t["ref_log_scale"], bounds=BOUNDS) if learned else dict(scale=L.SCALES[adim])
    return ops.laplace_dpo(t["pred"], t["ref_pred"], t["chosen"], t["rejected"], chunk, weight=t["weight"] if weight else None, want_dlog_scale=True, **scale, **kw)


def shipped(ops, t, learned, adim, adv, dev, on_ref=False, grad_scale=None):
    """The shipped group kernel on the pair as a group of two -> (logprob [rows, 2], dpred, dlog_scale or None)."""
    act = torch.stack([t["chosen"], t["rejected"]], dim=1).contiguous()
    pred = t["ref_pred"] if on_ref else t["pred"]
    if learned:
        out = ops.laplace_pg_rows(pred, t["ref_log_scale"] if on_ref else t["log_scale"], BOUNDS, act, adv, grad_scale=grad_scale)
        return out[0], out[5], out[6]
    out = ops.laplace_pg(pred, act, adv, L.SCALES[adim], grad_scale=grad_scale)
    return out[0], out[4], None


def twin_elems(w, learned, rows, adim):
    if learned:
        return S.elem_ref(w["s"], BOUNDS), S.elem_ref(w["ref_s"], BOUNDS)
    el = S.fixed_elem(L.SCALES[adim], rows, adim)
    return el, el


@pytest.mark.parametrize("learned", (False, True), ids=("fixed", "learned"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_the_shipped_kernels_and_the_twin(ops, dev, shape, learned):
    B, chunk, adim = shape
    rows = B * chunk
    w = D.dpo_inputs(B, chunk, adim, learned=learned)
    t = device_inputs(w, dev, learned, adim)
    elem, ref_elem = twin_elems(w, learned, rows, adim)
    ones = torch.ones((rows, 2), dtype=F32, device=dev)
    lp_want, rlp_want = shipped(ops, t, learned, adim, ones, dev)[0], shipped(ops, t, learned, adim, ones, dev, on_ref=True)[0]
    beta = beta_of(chunk, adim)
    for loss_type, nll_coef in VARIANTS:
        kw = dict(beta=beta, label_smoothing=0.1, loss_type=loss_type, grad_scale=1.0 / B, nll_coef=nll_coef, nll_scale=1.0 / rows)
        out = launch(ops, t, chunk, learned, adim, **kw)
        tag = f"{shape} {'learned' if learned else 'fixed'} {loss_type} nll {nll_coef}"
        assert out["logprob"].shape == (rows, 2) and out["h"].shape == (B, 2) and out["coef"].shape == (B,) and out["dpred"].dtype == BF
        # anchors: the log-probabilities are the shipped kernels' bits, on pred and on ref_pred
        same(out["logprob"], lp_want, f"{tag}: logprob vs the shipped kernel on pred")
        same(out["ref_logprob"], rlp_want, f"{tag}: ref_logprob vs the shipped kernel on ref_pred")
        # the twin, exact parts: h and the margin given those log-probabilities
        tw_kw = dict(weight=w["weight"], beta=beta, eps=0.1, loss_type=D.TYPES[loss_type], grad_scale=1.0 / B, nll_coef=nll_coef, nll_scale=1.0 / rows)
        twin = D.dpo_ref(w["mu"], w["ref_mu"], w["chosen"], w["rejected"], chunk, elem, ref_elem, logprob_bits=out["logprob"].cpu().numpy(),
                         ref_logprob_bits=out["ref_logprob"].cpu().numpy(), coef_bits=out["coef"].cpu().numpy(), **tw_kw)
        same_np(out["h"], twin["h"], f"{tag}: h"), same_np(out["margin"], twin["margin"], f"{tag}: margin")
        # the twin, bounded parts (IPO is IEEE: bit for bit)
        loss, coef = out["loss"].cpu().numpy(), out["coef"].cpu().numpy()
        assert bool(np.isfinite(loss).all()) and bool(np.isfinite(coef).all()) and bool(np.all(coef != 0)), f"{tag}: loss {loss}, coef {coef}"
        if loss_type == "ipo":
            same_np(out["loss"], twin["loss32"], f"{tag}: loss"), same_np(out["coef"], twin["coef32"], f"{tag}: coef")
        else:
            e_loss, e_coef = np.abs(loss.astype(np.float64) - twin["loss"]), np.abs(coef.astype(np.float64) - twin["coef"])
            z = beta * twin["margin"]
            print(f"{tag}: z in [{z.min():.2f}, {z.max():.2f}]; loss error / bound {float((e_loss / twin['loss_bound']).max()):.3f}, coef error / bound "
                  f"{float((e_coef / twin['coef_bound']).max()):.3f}")
            assert bool(np.all(e_loss <= twin["loss_bound"])), f"{tag}: loss error {e_loss} beyond the derived bound {twin['loss_bound']}"
            assert bool(np.all(e_coef <= twin["coef_bound"])), f"{tag}: coef error {e_coef} beyond the derived bound {twin['coef_bound']}"
        # the gradient given the kernel's own coef: the shipped kernel's G = 2 launch on (chosen, rejected) with (c_0, c_1), grad_scale 1
        adv = dv(np.repeat(twin["c"], chunk, axis=0), dev)
        if nll_coef > 0:
            assert bool(np.all(twin["c"][:, 0] != coef)), "the NLL term raises the chosen chunk's weight"
        _, dpred_want, dls_want = shipped(ops, t, learned, adim, adv, dev, grad_scale=1.0)
        same(out["dpred"], dpred_want, f"{tag}: dpred vs the shipped kernel at G = 2")
        assert bool((out["dpred"] != 0).any())
        if learned:
            same(out["dlog_scale"], dls_want, f"{tag}: dlog_scale vs the shipped kernel at G = 2")
        else:                                                      # a by-value scale: inv_b is the host's division, the twin's sums are exact
            assert np.array_equal(bits(out["dpred"]).numpy().view(np.uint16), twin["dpred_bits"]), f"{tag}: dpred vs the twin"
            assert np.array_equal(bits(out["dlog_scale"]).numpy().view(np.uint16), twin["dlog_scale_bits"]), f"{tag}: dlog_scale vs the twin"
    # without gradient outputs the per-observation outputs keep their bits; without the log-probability outputs too
    bare = launch(ops, t, chunk, learned, adim, beta=beta, label_smoothing=0.1, loss_type="ipo", grad_scale=None, nll_coef=0.5, nll_scale=1.0 / rows, want_logprob=False)
    assert bare["dpred"] is None and bare["logprob"] is None
    same(bare["h"], out["h"], "h without optional outputs"), same(bare["margin"], out["margin"], "margin without optional outputs"), same(bare["loss"], out["loss"], "loss")


@pytest.mark.parametrize("learned", (False, True), ids=("fixed", "learned"))
def test_an_observation_does_not_depend_on_its_position(ops, dev, learned):
    B, chunk, adim = 3, 8, 7
    w = D.dpo_inputs(B, chunk, adim, learned=learned)
    kw = dict(beta=beta_of(chunk, adim), label_smoothing=0.1, grad_scale=0.25, nll_coef=0.5, nll_scale=0.125)
    full = launch(ops, device_inputs(w, dev, learned, adim), chunk, learned, adim, **kw)

    def take(order):
        idx = np.concatenate([np.arange(b * chunk, (b + 1) * chunk) for b in order])
        sub = {k: (v[list(order)] if k == "weight" else v[idx]) for k, v in w.items()}
        return launch(ops, device_inputs(sub, dev, learned, adim), chunk, learned, adim, **kw)

    for order in ((1,), (2, 0, 1), (0,), (2,)):
        got = take(order)
        for i, b in enumerate(order):
            for k in ("logprob", "ref_logprob", "dpred", "dlog_scale"):
                same(got[k][i * chunk:(i + 1) * chunk], full[k][b * chunk:(b + 1) * chunk], f"order {order}: {k} of observation {b}")
            for k in ("h", "margin", "loss", "coef"):
                same(got[k][i:i + 1], full[k][b:b + 1], f"order {order}: {k} of observation {b}")


@pytest.mark.parametrize("learned", (False, True), ids=("fixed", "learned"))
def test_a_skipped_observation_may_hold_nan(ops, dev, learned):
    B, chunk, adim = 3, 8, 7
    w = D.dpo_inputs(B, chunk, adim, learned=learned)
    kw = dict(beta=beta_of(chunk, adim), label_smoothing=0.1, grad_scale=0.25, nll_coef=0.5, nll_scale=0.125)
    full = launch(ops, device_inputs(w, dev, learned, adim), chunk, learned, adim, **kw)
    hole = {k: v.copy() for k, v in w.items()}
    sl = slice(chunk, 2 * chunk)
    for k in ("mu", "ref_mu", "chosen", "rejected", "s", "ref_s"):
        hole[k][sl] = np.nan
    hole["weight"][1] = 0.0
    t = device_inputs(hole, dev, learned, adim)
    sentinel = lambda *shape, dt=F32: torch.full(shape, 7.0, dtype=dt, device=dev)   # noqa: E731  (a skipped observation's outputs are WRITTEN)
    rows = B * chunk
    got = launch(ops, t, chunk, learned, adim, logprob=sentinel(rows, 2), ref_logprob=sentinel(rows, 2), h=sentinel(B, 2), margin=sentinel(B), loss=sentinel(B),
                 coef=sentinel(B), dpred=sentinel(rows, adim, dt=BF), dlog_scale=sentinel(rows, adim, dt=BF), **kw)
    for k in ("logprob", "ref_logprob", "dpred", "dlog_scale"):
        assert not bits(got[k][sl]).any(), f"{k} of the skipped observation is not +0"
        same(got[k][:chunk], full[k][:chunk], f"{k} of observation 0"), same(got[k][2 * chunk:], full[k][2 * chunk:], f"{k} of observation 2")
    for k in ("h", "margin", "loss", "coef"):
        assert not bits(got[k][1]).any(), f"{k} of the skipped observation is not +0"
        same(got[k][[0, 2]], full[k][[0, 2]], f"{k} of the other observations")
    # coef == 0 with the NLL term off skips the gradient the same way: beta = 0 gives k = 0
    zero = launch(ops, device_inputs(w, dev, learned, adim), chunk, learned, adim, beta=0.0, grad_scale=0.25, dpred=sentinel(rows, adim, dt=BF),
                  dlog_scale=sentinel(rows, adim, dt=BF))
    assert not bits(zero["coef"]).any() and not bits(zero["dpred"]).any() and not bits(zero["dlog_scale"]).any()
    assert bool(((zero["loss"].cpu() - float(np.log(2.0))).abs() <= 4 * 2.0 ** -24).all()), "z = 0: the loss is ln 2 within logf's ulps"


def test_refusals(ops, dev):
    lib = importlib.import_module("openvla-oft_amd._lib")
    handle = lib.lib()
    cap_rows, cap_adim = 2 * 65, 17                               # every buffer holds the largest shape named below: nothing can leave one
    tens = dict(pred=torch.zeros((cap_rows, cap_adim), dtype=BF, device=dev), ref_pred=torch.zeros((cap_rows, cap_adim), dtype=BF, device=dev),
                log_scale=torch.zeros((cap_rows, cap_adim), dtype=BF, device=dev), ref_log_scale=torch.zeros((cap_rows, cap_adim), dtype=BF, device=dev),
                chosen=torch.ones((cap_rows, cap_adim), dtype=F32, device=dev), rejected=torch.zeros((cap_rows, cap_adim), dtype=F32, device=dev),
                weight=torch.ones(cap_rows, dtype=F32, device=dev), logprob=torch.zeros((cap_rows, 2), dtype=F32, device=dev),
                ref_logprob=torch.zeros((cap_rows, 2), dtype=F32, device=dev), h=torch.full((cap_rows, 2), 7.0, dtype=F32, device=dev),
                margin=torch.full((cap_rows,), 7.0, dtype=F32, device=dev), loss=torch.full((cap_rows,), 7.0, dtype=F32, device=dev),
                coef=torch.full((cap_rows,), 7.0, dtype=F32, device=dev), dpred=torch.full((cap_rows, cap_adim), 7.0, dtype=BF, device=dev),
                dlog_scale=torch.full((cap_rows, cap_adim), 7.0, dtype=BF, device=dev))

    def args(rows_form=False, **over):
        g = lib.STRUCTS["ovla_laplace_dpo_args"]()
        for k, v in tens.items():
            if k in ("log_scale", "ref_log_scale") and not rows_form:
                continue
            setattr(g, k, v.data_ptr())
        for d in range(16):
            g.scale[d], g.log_norm[d] = 1.0, float(np.log(2.0))
        g.s_lo, g.s_hi, g.beta, g.label_smoothing, g.grad_scale, g.nll_coef, g.nll_scale = -6.0, 1.0, 0.1, 0.1, 1.0, 0.5, 0.1
        g.loss_type, g.B, g.chunk, g.adim = 0, 2, 8, 7
        for k, v in over.items():
            if k == "scale0":
                g.scale[0] = v
            else:
                setattr(g, k, v)
        return g

    def refused(what, **over):
        rc = handle.ovla_laplace_dpo(ctypes.byref(args(**over)), None)
        assert rc == -1, f"{what}: rc = {rc}, OVLA_EINVAL expected"
        assert b"ovla_laplace_dpo" in handle.ovla_last_error(), f"{what}: {handle.ovla_last_error()}"

    nan, inf = float("nan"), float("inf")
    for name in ("pred", "ref_pred", "chosen", "rejected", "h", "margin", "loss", "coef"):
        refused(f"null {name}", **{name: None})
    for over in (dict(B=0), dict(B=-1), dict(chunk=0), dict(chunk=65), dict(adim=0), dict(adim=17)):
        refused(f"{over}", **over)
    refused("log_scale without ref_log_scale", log_scale=tens["log_scale"].data_ptr())
    refused("ref_log_scale without log_scale", ref_log_scale=tens["ref_log_scale"].data_ptr())
    for v in (0.0, -1.0, inf, nan):
        refused(f"scale {v}", scale0=v)
    for lo, hi in ((1.0, -6.0), (-inf, 1.0), (-6.0, inf), (nan, 1.0), (-6.0, nan)):
        refused(f"bounds {lo}, {hi}", rows_form=True, s_lo=lo, s_hi=hi)
    for v in (-1.0, nan, inf):
        refused(f"beta {v}", beta=v)
    for v in (-1.0, nan):
        refused(f"nll_coef {v}", nll_coef=v)
    for v in (-0.1, 0.5, nan):
        refused(f"label_smoothing {v}", label_smoothing=v)
    for v in (2, -1):
        refused(f"loss_type {v}", loss_type=v)
    refused("IPO with beta == 0", loss_type=1, beta=0.0)
    torch.cuda.synchronize(dev)
    for k in ("h", "margin", "loss", "coef", "dpred", "dlog_scale"):
        assert bool((tens[k] == 7.0).all()), f"a refused call wrote {k}"
    # the same arguments without the fault are taken, in both forms and at the cap
    for over in (dict(), dict(rows_form=True), dict(chunk=64, adim=16), dict(loss_type=1), dict(weight=None, logprob=None, ref_logprob=None, dpred=None, dlog_scale=None)):
        assert handle.ovla_laplace_dpo(ctypes.byref(args(**over)), None) == 0, f"{over}: {handle.ovla_last_error()}"
    torch.cuda.synchronize(dev)
    assert not bool((tens["h"][:2] == 7.0).any())
