"""Integer / float64 references and the test suites of the kernels that turn an observation into the decoder's input (csrc/elementwise.hip):
im2col_kernel, image_prep_kernel, assemble_kernel, language_average_kernel and its ragged form, transpose_batched_kernel, row_sumsq_kernel.
Nothing here needs a GPU.

These kernels are index arithmetic: they go wrong by a shifted row, a wrong channel or a write one element too far, not by an ulp.  So every
comparison is BIT EQUALITY OF WHOLE BUFFERS -- outputs sit inside sentinel-filled allocations and the allocation is compared, inputs sit inside
NaN-filled ones so that a read outside the operand shows in the result -- and the two kernels that add (language average, row_sumsq) are fed
small integers, whose fp32 sums are exact in any order.  There is no tolerance anywhere in this file.

Each suite takes a `Failures` and an object K whose methods run one kernel on CPU tensors and return CPU tensors: tests/test_input_path_gpu.py
passes the real launches, tests/test_input_path_reference.py a restatement of the kernels with and without planted bugs.  Shapes and data are
decided here, once, for both.  The interface:

  K.im2col(px, c0, patch, ldo, n_img, img_cstride, out)          out: Slab [rows, ldo]            -> the whole allocation of `out`
  K.image_prep(frames, n, crop, crop_scale, out_size)            frames uint8 [n + 1, H, W, 3]     -> bf16 [1, 6 n, out, out] of frames[:n]
  K.assemble(ids, labels, table, patches, noisy, A, out, apos)   table / out / apos: Slabs         -> the allocations of `out` and `apos`
  K.language_average(ids, labels, B, lens, table, out)           ids / labels [B + 1, L], row B a guard; lens None: the plain kernel
  K.transpose_batched(pairs)                                     [(src, dst)] of gemm_reference.Embedded -> the allocations of the dsts
  K.row_sumsq(src, dim, out)                                     src: Embedded [rows, dim]; out: Slab fp32 [rows, dim / 64]
"""
import math

import numpy as np
import torch

from tests.gemm_reference import BF, SENTINEL, Embedded, Failures, embed, ints, rng  # noqa: F401
from tests.pointwise_reference import GRID_CAP_ITEMS, _sent, masked_mean_ref, randn_bf, same_bits  # noqa: F401

IGNORE, STOP, ACTION_BEGIN = -100, 2, 31743           # labels: not a label / the stop token / labels above this are action tokens
IMAGE_MEAN, IMAGE_STD = (0.485, 0.456, 0.406, 0.5, 0.5, 0.5), (0.229, 0.224, 0.225, 0.5, 0.5, 0.5)
NAN_BITS = 0x7FC0                                     # the quiet NaN the guards of bf16 inputs hold
BIG_ID = 2 ** 40


class Slab:
    """A CONTIGUOUS tensor of `shape` inside a flat allocation with `pad` guard elements before and after it (for the operands these kernels
    address without a leading dimension): `buf` is the allocation, `view` the tensor.  `fill`: "sentinel" (outputs) | "nan" (inputs)."""

    def __init__(self, dtype, shape, fill="sentinel", pad=64, src=None, buf=None):
        self.shape, self.pad, self.n = tuple(shape), pad, math.prod(shape)
        if buf is None:
            buf = torch.empty(self.n + 2 * pad, dtype=dtype)
            if fill == "sentinel":
                buf.view(torch.int16 if buf.element_size() == 2 else torch.int32).fill_(SENTINEL[buf.element_size()])
            else:
                buf.fill_(float("nan"))
        self.buf = buf
        self.view = buf[pad:pad + self.n].view(self.shape)
        assert (pad * buf.element_size()) % 16 == 0 and self.view.data_ptr() % 16 == 0
        if src is not None:
            self.view.copy_(src)

    def on(self, device):
        """The same layout with the allocation copied to `device`."""
        return Slab(self.buf.dtype, self.shape, pad=self.pad, buf=self.buf.to(device))


def rows_embed(x, ld, top=3, bottom=5):
    """x [rows, dim] as the first `dim` columns of rows `top` .. of a NaN-filled [top + rows + bottom, ld] allocation: the leading dimension is
    exactly `ld` (ld == dim: guard rows only)."""
    rows, dim = x.shape
    assert ld >= dim
    buf = torch.full((top + rows + bottom, ld), float("nan"), dtype=x.dtype)
    e = Embedded(buf, top, 0, rows, dim)
    e.view.copy_(x)
    return e


def random_bits_bf(g, shape):
    """Every bf16 bit pattern, NaN payloads and infinities included: these kernels move bits."""
    return torch.randint(-32768, 32768, shape, generator=g, dtype=torch.int32).to(torch.int16).view(BF)


# ---- im2col ------------------------------------------------------------------------------------------------------------------------------------
IM2COL_CASES = ((1, 3, 0, 1, 6, 14, 14, 14, 588),        # one patch, ldo == kreal exactly
                (2, 12, 3, 2, 6, 28, 42, 14, 592),       # two images per batch row, H != W
                (3, 12, 0, 2, 6, 32, 16, 16, 776),       # patch 16
                (2, 9, 0, 3, 3, 28, 28, 14, 592))        # channel stride 3, three images
IM2COL_WRAP = (4, 12, 3, 2, 6, 224, 224, 14, 592)        # 1,212,416 work items: a second trip of the grid-stride loop with n_img > 1


def im2col_ref(px, c0, patch, ldo, n_img, img_cstride):
    """torch.nn.functional.unfold on the selected channels of every image, zero-padded to ldo.  Done on the 16-bit patterns (exact in fp32), so
    NaN payloads survive."""
    B, _, H, W = px.shape
    bits = px.view(torch.int16).to(torch.int32) & 0xFFFF
    per_img = []
    for img in range(n_img):
        c = c0 + img * img_cstride
        u = torch.nn.functional.unfold(bits[:, c:c + 3].float(), kernel_size=patch, stride=patch)          # [B, 3 p p, gh gw]
        per_img.append(u.transpose(1, 2))
    cols = torch.stack(per_img, 1).reshape(-1, 3 * patch * patch).to(torch.int32)
    cols = torch.cat([cols, torch.zeros((cols.shape[0], ldo - cols.shape[1]), dtype=torch.int32)], 1)
    return cols.to(torch.int16).view(BF)


def suite_im2col(fails, K, cap=GRID_CAP_ITEMS, cases=IM2COL_CASES, wrap=IM2COL_WRAP):
    for n, case in enumerate(tuple(cases) + ((wrap,) if wrap else ())):
        B, C, c0, n_img, cstride, H, W, patch, ldo = case
        g = rng(1100 + n)
        px = random_bits_bf(g, (B, C, H, W))
        used = torch.zeros(C, dtype=torch.bool)
        for img in range(n_img):
            used[c0 + img * cstride:c0 + img * cstride + 3] = True
        px.view(torch.int16)[:, ~used] = NAN_BITS                 # channels outside the selected ones hold NaN
        rows = B * n_img * (H // patch) * (W // patch)
        if case == wrap:
            assert rows * ldo > cap, "the wrap case must need a second trip"
        out = Slab(BF, (rows, ldo))
        want = out.buf.clone()
        want[out.pad:out.pad + out.n] = im2col_ref(px, c0, patch, ldo, n_img, cstride).flatten()
        same_bits(fails, K.im2col(px, c0, patch, ldo, n_img, cstride, out), want,
                  f"im2col B {B} C {C} c0 {c0} n_img {n_img} cstride {cstride} {H}x{W} patch {patch} ldo {ldo} (whole allocation)")


# ---- image_prep --------------------------------------------------------------------------------------------------------------------------------
# (H, W, out, crop_scale or None for crop off, frames)
PREP_RUN = ((224, 224, 224, 0.9, 3), (256, 320, 224, 0.9, 3), (256, 256, 224, 0.9, 2), (224, 224, 224, None, 3))
PREP_OVERSHOOT = tuple((H, W, o, s, 2) for H, W, o in ((480, 480, 384), (100, 100, 96), (30, 30, 224), (30, 100, 45)) for s in (1.0, 1.5))
PREP_SMALL = ((2, 2, 2, 0.5, 2),)
PREP_WRAP = ((224, 224, 224, None, 22), (224, 224, 224, 0.9, 22))          # 22 * 224 * 224 = 1,103,872 pixels > 1,048,576
_prep_cache = {}


def prep_frames(H, W, n, seed):
    """n + 1 frames: the first n random and all different, with a saturated top band in frame 0 and a black left band in frame 1; the last one,
    which no launch is given, all 255 -- a read one row or one pixel past frame n - 1 lands there and shows."""
    r = np.random.default_rng(seed)
    fr = r.integers(0, 256, (n + 1, H, W, 3), dtype=np.uint8)
    fr[0, :max(1, H // 28)] = 255
    if n > 1:
        fr[1, :, :max(1, W // 28)] = 0
    fr[n] = 255
    return torch.from_numpy(fr)


def image_prep_ref(frames, n, crop_scale, out_size):
    """oracle.vla_oracle: crop_and_resize_center (crop on) + image_transform, frame by frame -> (bf16 [1, 6 n, out, out], the uint8 crops)."""
    from oracle import vla_oracle as vo

    qs, ref = [], []
    for im in frames[:n].numpy():
        q = im if crop_scale is None else vo.crop_and_resize_center(im, crop_scale, out_size)
        qs.append(q)
        ref.append(vo.image_transform(q, (vo.IMAGENET_MEAN, vo.SIGLIP_MEAN), (vo.IMAGENET_STD, vo.SIGLIP_STD)))
    return torch.cat(ref, 0)[None].to(BF), np.stack(qs)


def prep_case(case):
    """Frames and reference of one case, computed once and shared (never modified)."""
    if case not in _prep_cache:
        H, W, out, scale, n = case
        frames = prep_frames(H, W, n, 1200 + H * 7 + W + out + n)
        _prep_cache[case] = (frames,) + image_prep_ref(frames, n, scale, out)
    return _prep_cache[case]


def suite_image_prep(fails, K, cap=GRID_CAP_ITEMS, cases=PREP_RUN + PREP_OVERSHOOT + PREP_SMALL, wrap=PREP_WRAP):
    for case in tuple(cases) + tuple(wrap):
        H, W, out, scale, n = case
        frames, ref, q = prep_case(case)
        what = f"image_prep {n} x {H}x{W} -> {out} crop_scale {scale}"
        if case in wrap:
            assert n * out * out > cap, "the wrap case must need a second trip"
            assert len({fr.tobytes() for fr in frames[:n].numpy()}) == n, "every frame must be different"
        if case in PREP_OVERSHOOT:
            # the last sampling coordinate rounds above H - 1 (or W - 1): TF's extrapolation_value.  Without this the case could pass vacuously.
            fails.check(bool((q[:, -1] == 0).all() or (q[:, :, -1] == 0).all()), what + ": the reference has no black last row or column")
        same_bits(fails, K.image_prep(frames, n, scale is not None, 0.9 if scale is None else scale, out), ref, what)


# ---- multimodal assembly -----------------------------------------------------------------------------------------------------------------------
ASSEMBLE_SHAPES = ((1, 1, 1, 8), (3, 12, 5, 264), (2, 9, 3, 2056))      # (B, L, P, D); D = 2056: a second trip of the 256 x 8 column loop
ASSEMBLE_A = (1, 4)
ASSEMBLE_VOCAB = 37
ASSEMBLE_CASES = ("exactly A", "A + 2", "A - 3", "none", "at index 0", "other labels", "edge ids")


def assemble_ref(ids, labels, table, patches, noisy, A, ignore_index=IGNORE, action_begin=ACTION_BEGIN):
    """modeling_prismatic.py:571-629 with train_utils.py:8-39's action mask, position by position: out [B, P + L, D] and action_pos [B, A]
    (-1 where the labels hold fewer than A action tokens).  Ids are clamped to the table; an action position's embedding is replaced by its
    slot's row of `noisy`, or by zeros without `noisy` or for a slot >= A."""
    B, L = ids.shape
    V, D = table.shape
    P = patches.shape[1]
    S = P + L
    out = torch.zeros((B, S, D), dtype=BF)
    apos = torch.full((B, A), -1, dtype=torch.int32)
    for b in range(B):
        seen, slot = False, 0
        out[b, 1:1 + P] = patches[b]
        for i in range(L):
            lab = int(labels[b, i])
            seen = seen or lab != ignore_index
            row = 0 if i == 0 else P + i
            if seen and lab > action_begin:
                if slot < A:
                    apos[b, slot] = b * S + P + i - 1
                    if noisy is not None:
                        out[b, row] = noisy[b, slot]
                slot += 1
            else:
                out[b, row] = table[min(max(int(ids[b, i]), 0), V - 1)]
    return out, apos


def assemble_case(g, name, B, L, A, V):
    """ids / labels of one case, or None where L has no room for it.  Prompts are ragged; action tokens are labels above ACTION_BEGIN."""
    n_act = {"exactly A": A, "A + 2": A + 2, "A - 3": max(A - 3, 0), "none": 0, "at index 0": min(A, L), "other labels": A, "edge ids": A}[name]
    lead = 1 if name == "other labels" else 0                      # a counted label that is no action token, BEFORE the action tokens
    if n_act + lead > L or (name == "edge ids" and L < n_act + 3):
        return None
    ids = torch.randint(0, V, (B, L), generator=g)
    labels = torch.full((B, L), IGNORE, dtype=torch.int64)
    for b in range(B):
        room = L - n_act
        start = 0 if name == "at index 0" else max(lead, min(room - 1, 1 + b % 2 + lead)) if room > 0 else 0
        if name == "edge ids":
            start = max(start, 3)
        labels[b, start:start + n_act] = ACTION_BEGIN + 1 + torch.randint(0, 256, (n_act,), generator=g)
        if lead:
            labels[b, start - 1] = 29871                            # counted, not an action: embedded normally, takes no slot
        if start + n_act < L:
            labels[b, start + n_act] = STOP                         # the stop token: likewise
        if name == "none" and b % 2:
            labels[b] = IGNORE                                      # ... and a row with no label at all
    if name == "edge ids":
        ids[:, 0], ids[:, 1], ids[:, 2] = -1, V, BIG_ID             # clamped to rows 0, V - 1, V - 1
    return ids, labels


def suite_assemble(fails, K, shapes=ASSEMBLE_SHAPES, As=ASSEMBLE_A, cases=ASSEMBLE_CASES):
    V = ASSEMBLE_VOCAB
    ran = set()
    for B, L, P, D in shapes:
        for A in As:
            g = rng(1300 + D + A)
            table = Slab(BF, (V, D), fill="nan", pad=4 * D, src=randn_bf(g, (V, D)))           # four NaN guard rows above and below
            patches, noisy_rows = randn_bf(g, (B, P, D)), randn_bf(g, (B, A, D))
            for name in cases:
                c = assemble_case(g, name, B, L, A, V)
                if c is None:
                    continue
                ran.add(name)
                ids, labels = c
                for noisy in (None, noisy_rows):
                    want_out, want_pos = assemble_ref(ids, labels, table.view, patches, noisy, A)
                    out, apos = Slab(BF, (B, P + L, D)), Slab(torch.int32, (B, A))
                    apos.view.fill_(-1)
                    wo, wp = out.buf.clone(), apos.buf.clone()
                    wo[out.pad:out.pad + out.n] = want_out.flatten()
                    wp[apos.pad:apos.pad + apos.n] = want_pos.flatten()
                    got_out, got_pos = K.assemble(ids, labels, table, patches, noisy, A, out, apos)
                    what = f"assemble B {B} L {L} P {P} D {D} A {A} '{name}' noisy {noisy is not None}"
                    same_bits(fails, got_out, wo, what + ": out (whole allocation)")
                    same_bits(fails, got_pos, wp, what + ": action_pos (whole allocation, pre-filled with -1)")
    assert ran == set(cases), f"cases that fitted no shape: {set(cases) - ran}"


# ---- language average --------------------------------------------------------------------------------------------------------------------------
LANG_DIMS = (8, 264, 520)
LANG_L, LANG_VOCAB, LANG_NAN_ROW = 9, 23, 11
LANG_LENS = ((1, 9, 0, -3, 14), (9, 0, -3, 14, 1), (4, 5, 6, 7, 3))       # {1, L, 0, -3, L + 5} on different rows, and lengths inside the row


def language_rows(g):
    """Five rows of LANG_L positions: one text position (index 0) | none | all text | ids -1, vocab, 2^40 | labels at ACTION_BEGIN exactly."""
    B, L, V = 5, LANG_L, LANG_VOCAB
    ids = torch.randint(0, V, (B, L), generator=g)
    ids[ids == LANG_NAN_ROW] = 0
    labels = torch.full((B, L), ACTION_BEGIN + 7, dtype=torch.int64)
    labels[0, 0] = IGNORE
    labels[2] = IGNORE
    labels[3, :6] = IGNORE
    ids[3, 0], ids[3, 2], ids[3, 4] = -1, V, BIG_ID
    labels[4, :5] = torch.tensor([IGNORE, ACTION_BEGIN, ACTION_BEGIN + 1, STOP, ACTION_BEGIN])       # <= ACTION_BEGIN is text
    return ids, labels


def language_average_ref(ids, labels, lens, table):
    """Mean of the (clamped) ids' table rows over positions i < clamp(lens, 0, L) with labels <= ACTION_BEGIN: masked_mean_ref's convention,
    bf16(fl32(sum) / fl32(max(count, 1))); the sum of small integers is exact."""
    B, L = ids.shape
    V, D = table.shape
    n = torch.full((B,), L) if lens is None else torch.tensor(lens).clamp(0, L)
    mask = ((labels <= ACTION_BEGIN) & (torch.arange(L)[None] < n[:, None])).to(torch.uint8)
    x = table[ids.clamp(0, V - 1)]
    x = torch.where(mask.bool()[..., None], x, torch.zeros_like(x))             # what the mask excludes may be NaN
    return masked_mean_ref(x, mask, B, L, D)


def suite_language_average(fails, K, dims=LANG_DIMS):
    V, L = LANG_VOCAB, LANG_L
    for D in dims:
        g = rng(1400 + D)
        rows = ints(g, (V, D), -8, 8)
        rows[LANG_NAN_ROW] = float("nan")                          # a row of the table itself: what the positions beyond lens point at
        table = Slab(BF, (V, D), fill="nan", pad=4 * D, src=rows)
        ids, labels = language_rows(g)
        B = ids.shape[0]
        for lens in (None,) + LANG_LENS:
            i, lab = ids.clone(), labels.clone()
            if lens is not None:
                for b, n in enumerate(lens):
                    n = min(max(n, 0), L)
                    i[b, n:], lab[b, n:] = LANG_NAN_ROW, IGNORE     # beyond the row: a text position pointing at NaN
            guard_i, guard_l = torch.full((1, L), LANG_NAN_ROW), torch.full((1, L), IGNORE)      # row B of the allocations: likewise
            want = language_average_ref(i, lab, lens, table.view)
            fails.check(bool(torch.isfinite(want.float()).all()), f"language average D {D} lens {lens}: the reference is not finite")
            fails.check(bool((want[1] == 0).all()), f"language average D {D}: a row without a text position gives zeros")
            out = Slab(BF, (B + 2, D))
            w = out.buf.clone()
            w[out.pad:out.pad + B * D] = want.flatten()             # rows out[B:] keep the sentinel
            got = K.language_average(torch.cat([i, guard_i]), torch.cat([lab, guard_l]), B, None if lens is None else torch.tensor(lens, dtype=torch.int32), table, out)
            same_bits(fails, got, w, f"language average {'plain' if lens is None else 'ragged'} D {D} lens {lens} (whole allocation)")


# ---- batched transpose -------------------------------------------------------------------------------------------------------------------------
TRANSPOSE_ENTRIES = ((1, 1), (64, 64), (63, 65), (65, 63), (130, 1), (1, 130), (96, 300), (520, 32), (64, 64))


def suite_transpose_batched(fails, K, entries=TRANSPOSE_ENTRIES):
    g = rng(1500)
    pairs, wants = [], []
    for rows, cols in entries:
        src = embed(randn_bf(g, (rows, cols)), align=4, fill="nan")
        dst = embed(BF, shape=(cols, rows), align=4, fill="sentinel", device="cpu")
        want = dst.buf.clone()
        want[dst.r0:dst.r0 + cols, dst.c0:dst.c0 + rows] = src.view.T
        pairs.append((src, dst))
        wants.append(want)
    order = list(range(len(entries)))
    for name, sel in (("nine entries", order), ("reversed", order[::-1]), ("one entry", [6])):
        got = K.transpose_batched([pairs[i] for i in sel])
        for i, o in zip(sel, got):
            same_bits(fails, o, wants[i], f"transpose_batched {name}: entry {entries[i][0]}x{entries[i][1]} (position {sel.index(i)}; whole destination buffer)")


# ---- row_sumsq ---------------------------------------------------------------------------------------------------------------------------------
SUMSQ_CASES = ((1, 64, 64), (5, 128, 136), (7, 4160, 4168), (4, 4096, 4096))      # (rows, dim, ld); 4160: 65 slots, lane 0 runs its second


def suite_row_sumsq(fails, K, cases=SUMSQ_CASES):
    for rows, dim, ld in cases:
        g = rng(1600 + dim)
        x = ints(g, (rows, dim), -4, 4)                            # 64 squares of at most 16: every fma of the chain is exact
        src = rows_embed(x, ld)
        out = Slab(torch.float32, (rows, dim // 64))
        want = out.buf.clone()
        want[out.pad:out.pad + out.n] = x.double().view(rows, dim // 64, 64).pow(2).sum(-1).float().flatten()
        same_bits(fails, K.row_sumsq(src, dim, out), want, f"row_sumsq rows {rows} dim {dim} ld {ld} (whole allocation)")
