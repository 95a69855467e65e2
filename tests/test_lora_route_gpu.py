"""The two routing kernels of multi-adapter serving (csrc/lora_route.hip), bit for bit against numpy: ovla_lora_route zeroes, per row, the
projection columns of every adapter slot but the row's own; ovla_select_by_slot picks each observation's own policy's rows."""
import importlib

import numpy as np
import pytest
import torch

load = importlib.import_module
BF = torch.bfloat16
R = 32
NAN, SENTINEL = 0x7FC0, 0x4321   # bf16 bit patterns: a quiet NaN, and an ordinary value for the pad columns


def _bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


def _route_ref(t, ld, slots, G, n, rows_per_obs):
    """numpy restatement on uint16 bit patterns: +0 over every column of a foreign slot, nothing else touched."""
    out = t.copy()
    for m in range(t.shape[0]):
        own = slots[m // rows_per_obs]
        for g in range(G):
            for s in range(n):
                if s != own:
                    out[m, (g * n + s) * R:(g * n + s + 1) * R] = 0
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("M,rows_per_obs", [(70, 14), (1, 14)])
@pytest.mark.parametrize("n", [1, 2, 4])
@pytest.mark.parametrize("G", [1, 3])
def test_lora_route_matches_numpy(dev, ops, G, n, M, rows_per_obs):
    rng = np.random.default_rng(100 * G + 10 * n + M)
    width, ld = G * n * R, G * n * R + 8
    n_obs = (M + rows_per_obs - 1) // rows_per_obs
    slots = [int(v) for v in rng.integers(0, n, n_obs)]
    if n > 1 and n_obs > 1:
        slots[0], slots[1] = n - 1, 0          # the slot changes inside the first wavefront's rows
    host = torch.randn(M, ld, generator=torch.Generator().manual_seed(M + n)).to(BF)
    h = host.view(torch.int16).numpy().view(np.uint16).copy()
    h[:, width:] = SENTINEL
    own0, foreign0 = slots[0], (slots[0] + 1) % n
    h[0, (0 * n + own0) * R + 3] = NAN                     # in the row's own columns: must survive
    if n > 1:
        h[0, ((G - 1) * n + foreign0) * R + 5] = NAN       # in a foreign slot's columns: must come out as zero
    t = torch.from_numpy(h.view(np.int16).copy()).view(BF).to(dev)
    obs_slot = torch.tensor(slots, dtype=torch.int32, device=dev)
    ops.lora_route(t, obs_slot, G=G, n=n, r=R, rows_per_obs=rows_per_obs, host_slots=slots)
    torch.cuda.synchronize()
    got, want = _bits(t), _route_ref(h, ld, slots, G, n, rows_per_obs)
    assert np.array_equal(got, want)
    assert (got[:, width:] == SENTINEL).all(), "pad columns untouched"
    assert got[0, (0 * n + own0) * R + 3] == NAN
    if n > 1:
        assert got[0, ((G - 1) * n + foreign0) * R + 5] == 0, "stored zero, not NaN * 0"


@pytest.mark.gpu
def test_lora_route_out_of_range_slots(dev, ops):
    """A slot outside [0, n) is OVLA_EINVAL where the host sees the values; the kernel clamps what it reads from the device array."""
    _lib = load("openvla-oft_amd._lib")
    G, n, M, rpo = 3, 2, 70, 14
    width = G * n * R
    src = torch.randn(M, width, generator=torch.Generator().manual_seed(1)).to(BF)
    for bad in ([0, 1, n, 0, 1], [0, -1, 1, 0, 1]):
        t = src.clone().to(dev)
        obs_slot = torch.tensor(bad, dtype=torch.int32, device=dev)
        with pytest.raises(_lib.OvlaError, match="obs_slot"):
            ops.lora_route(t, obs_slot, G=G, n=n, r=R, rows_per_obs=rpo, host_slots=bad)
        torch.cuda.synchronize()
        assert torch.equal(t.cpu(), src), "nothing was launched"
        ops.lora_route(t, obs_slot, G=G, n=n, r=R, rows_per_obs=rpo)          # device values only: clamped to [0, n)
        torch.cuda.synchronize()
        clamped = [min(max(v, 0), n - 1) for v in bad]
        assert np.array_equal(_bits(t), _route_ref(_bits(src), width, clamped, G, n, rpo))
    with pytest.raises(_lib.OvlaError):      # more rows than obs_slot covers
        ops.lora_route(src.clone().to(dev), torch.zeros(4, dtype=torch.int32, device=dev), G=G, n=n, r=R, rows_per_obs=rpo)


@pytest.mark.gpu
@pytest.mark.parametrize("rows_per_obs", [1, 8])
@pytest.mark.parametrize("dim", [7, 56, 1024])
@pytest.mark.parametrize("dtype", [BF, torch.float32])
def test_select_by_slot_matches_numpy(dev, ops, dtype, dim, rows_per_obs):
    _lib = load("openvla-oft_amd._lib")
    n, B = 3, 5
    rows = B * rows_per_obs
    src = torch.randn(n, rows + 3, dim, generator=torch.Generator().manual_seed(dim + rows_per_obs)).to(dtype)   # 3 padding rows per slot
    slots = [2, 0, 1, 1, 2]
    obs_slot = torch.tensor(slots, dtype=torch.int32, device=dev)
    got = ops.select_by_slot(src.to(dev), obs_slot, rows_per_obs=rows_per_obs, rows=rows, host_slots=slots)
    want = torch.stack([src[slots[m // rows_per_obs], m] for m in range(rows)])
    assert got.shape == (rows, dim) and torch.equal(got.cpu().view(torch.int16 if dtype == BF else torch.int32), want.view(torch.int16 if dtype == BF else torch.int32))
    bad = [2, 0, 3, -1, 2]
    bad_dev = torch.tensor(bad, dtype=torch.int32, device=dev)
    with pytest.raises(_lib.OvlaError, match="obs_slot"):
        ops.select_by_slot(src.to(dev), bad_dev, rows_per_obs=rows_per_obs, rows=rows, host_slots=bad)
    got = ops.select_by_slot(src.to(dev), bad_dev, rows_per_obs=rows_per_obs, rows=rows)      # clamped on the device: slots 2, 0, 2, 0, 2
    clamped = [min(max(v, 0), n - 1) for v in bad]
    assert torch.equal(got.cpu(), torch.stack([src[clamped[m // rows_per_obs], m] for m in range(rows)]))
