"""Per-policy FiLM without a GPU: every argument check of ovla_film_vectors returns OVLA_EINVAL before anything is launched (fake, aligned
addresses are enough: nothing dereferences a device pointer), and the slot layout the engine writes (engine.fill_film_slot, the table order of
engine.film_linear_names) restated in numpy against float64."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

load = importlib.import_module
EINVAL = -1


@pytest.fixture(scope="module")
def lib(pkg):
    return load("openvla-oft_amd._lib")


def _call(lib, *, n_linears=2, out_fs=(128, 5), D=256, n=2, n_obs=3, host_slots=None, patch=None, patch_linear=None):
    """A valid call description with one thing changed; -> (rc, message).  Device addresses are fake multiples of 256."""
    T, A = lib.STRUCTS["ovla_film_linear"], lib.STRUCTS["ovla_film_vectors_args"]
    arr = (T * max(n_linears, 1))()
    start = 0
    for j in range(n_linears):
        arr[j].W, arr[j].bias, arr[j].out = 0x10000 * (j + 1), 0x10000 * (j + 1) + 0x4000, 0x10000 * (j + 1) + 0x8000
        arr[j].out_f, arr[j].item_start = out_fs[j], start
        start += (out_fs[j] + 3) // 4
    if patch_linear is not None:
        patch_linear(arr)
    g = A()
    g.table, g.table_host = 0x900000, ctypes.cast(arr, ctypes.c_void_p).value
    g.avg, g.ld_avg, g.obs_slot = 0xA00000, D, 0xB00000
    hs = None
    if host_slots is not None:
        hs = (ctypes.c_int32 * len(host_slots))(*host_slots)
        g.obs_slot_host = ctypes.cast(hs, ctypes.c_void_p).value
    g.n_linears, g.n_obs, g.n, g.D = n_linears, n_obs, n, D
    if patch is not None:
        patch(g)
    rc = lib.lib().ovla_film_vectors(ctypes.byref(g), None)
    return rc, lib.lib().ovla_last_error().decode()


def _set(**kw):
    def patch(g):
        for k, v in kw.items():
            setattr(g, k, v)
    return patch


def _set_linear(j, **kw):
    def patch(arr):
        for k, v in kw.items():
            setattr(arr[j], k, v)
    return patch


@pytest.mark.parametrize("patch,word", [
    (_set(table=None), "null"), (_set(table_host=None), "null"), (_set(avg=None), "null"), (_set(obs_slot=None), "null"),
    (_set(D=260), "D = 260"), (_set(D=0), "D = 0"), (_set(ld_avg=252), "ld_avg"), (_set(ld_avg=258), "ld_avg"),
    (_set(n=0), "n = 0"), (_set(n=5), "n = 5"), (_set(n_obs=0), "n_obs = 0"), (_set(n_obs=65), "n_obs = 65"),
    (_set(n_linears=0), "n_linears = 0"), (_set(avg=0xA00008), "avg"), (_set(obs_slot=0xB00002), "obs_slot"),
])
def test_argument_refusals(lib, patch, word):
    rc, msg = _call(lib, patch=patch)
    assert rc == EINVAL and "ovla_film_vectors" in msg and word in msg, msg


@pytest.mark.parametrize("patch,word", [
    (_set_linear(1, out_f=0), "out_f = 0"), (_set_linear(0, out_f=-4), "out_f = -4"), (_set_linear(0, W=None), "null"),
    (_set_linear(1, bias=None), "null"), (_set_linear(1, out=None), "null"), (_set_linear(0, W=0x10008), "16-byte"),
    (_set_linear(1, bias=0x24001), "2-byte"), (_set_linear(1, out=0x28001), "2-byte"), (_set_linear(1, item_start=31), "item_start"),
])
def test_host_table_refusals(lib, patch, word):
    rc, msg = _call(lib, patch_linear=patch)
    assert rc == EINVAL and "ovla_film_vectors: linear" in msg and word in msg, msg


@pytest.mark.parametrize("slots", [[0, 2, 1], [0, -1, 1], [7, 0, 0]])
def test_host_slots_out_of_range(lib, slots):
    rc, msg = _call(lib, host_slots=slots)
    assert rc == EINVAL and "obs_slot[" in msg and "outside [0, 2)" in msg, msg


def test_slot_layout_against_numpy(pkg):
    """W_slots [n, dim, D] / b_slots [n, dim] as engine.fill_film_slot writes them, in the table order of engine.film_linear_names, against
    gamma / beta = Linear_{slot(b)}(avg[b]) in float64 for every block of both towers."""
    engine = load("openvla-oft_amd.engine")
    rng = np.random.default_rng(0)
    D, n, B = 24, 3, 5
    towers = [("vision_backbone.featurizer.", 2, 16), ("vision_backbone.fused_featurizer.", 3, 12)]   # (prefix, used blocks, dim)
    names = engine.film_linear_names(towers)
    assert names[:4] == ["vision_backbone.featurizer.blocks.0.scale", "vision_backbone.featurizer.blocks.0.shift",
                         "vision_backbone.featurizer.blocks.1.scale", "vision_backbone.featurizer.blocks.1.shift"]
    assert len(names) == 2 * (2 + 3) and names[4] == "vision_backbone.fused_featurizer.blocks.0.scale"
    dims = {nm: (16 if ".featurizer." in nm and "fused" not in nm else 12) for nm in names}
    policies = [{f"{nm}.{leaf}": rng.standard_normal((dims[nm], D) if leaf == "weight" else (dims[nm],)) for nm in names for leaf in ("weight", "bias")}
                for _ in range(n)]
    W_slots = {nm: torch.zeros(n, dims[nm], D, dtype=torch.float64) for nm in names}
    b_slots = {nm: torch.zeros(n, dims[nm], dtype=torch.float64) for nm in names}
    for s, pol in enumerate(policies):
        for nm in names:
            engine.fill_film_slot(W_slots[nm], b_slots[nm], s, torch.from_numpy(pol[nm + ".weight"]), torch.from_numpy(pol[nm + ".bias"]))
    avg, slots = rng.standard_normal((B, D)), rng.integers(0, n, B)
    for nm in names:   # ovla_film_vectors: out[b] = bias[slot(b)] + W[slot(b)] . avg[b]
        W, b = W_slots[nm].numpy(), b_slots[nm].numpy()
        got = np.stack([b[slots[i]] + W[slots[i]] @ avg[i] for i in range(B)])
        want = np.stack([policies[slots[i]][nm + ".bias"] + policies[slots[i]][nm + ".weight"] @ avg[i] for i in range(B)])
        assert got.shape == (B, dims[nm]) and np.allclose(got, want, rtol=1e-12, atol=1e-12)
