"""The suites of tests/input_path_reference.py discriminate (no GPU).

`Emulated` restates the input-path kernels of csrc/elementwise.hip -- im2col, image_prep, assemble, the two language averages, the batched
transpose, row_sumsq -- on the CPU, index for index (flat offsets into the same allocations the kernels are handed, so a read or a write
outside an operand lands where the kernel's would), behind the interface the suites drive.  tests/test_input_path_gpu.py hands the same suites
the real launches; here

* the correct restatement passes every suite (the two grid-stride cases at a cap of 4096 work items instead of 1,048,576: the same data);
* each planted bug (`MUTATIONS`) is rejected, by the suite and the check meant to catch it;
* the restatement without the extrapolation rule -- image_prep_kernel as it was -- fails suite_image_prep at the four overshoot shapes and
  nowhere else;
* for each bug, the inputs of the tests that covered these kernels before (test_vision_front_end_glue, test_assemble_and_gather,
  test_image_prep_bit_exact_vs_oracle, the batched-transpose lines of test_gemm_tn_grouped_and_block_diagonal, the row_sumsq line of
  test_gemm_rmsnorm_fold, test_ragged_average_gpu.py) are run through the mutated restatement with those tests' own assertions; whether they
  accept it is pinned in `OLD_TESTS_ACCEPT` and printed;
* vla_oracle.crop_and_resize_center and data_oracle.crop_and_resize mark the same pixels as outside the image.
"""
import numpy as np
import pytest
import torch

from tests import input_path_reference as R

BF = torch.bfloat16
F32 = np.float32


def _flat_take(flat, start, n, nan):
    """flat[start : start + n], with `nan` where that leaves the allocation (an emulated read there has no defined value)."""
    if 0 <= start and start + n <= flat.numel():
        return flat[start:start + n]
    return torch.full((n,), nan, dtype=flat.dtype)


class Emulated:
    """The kernels restated on CPU tensors.  `mut` plants one bug; `cap` is the number of work items one trip of a grid-stride loop covers (the
    real kernels: 1,048,576)."""

    def __init__(self, mut=None, cap=4096):
        self.mut, self.cap = mut, cap

    # ---- im2col_kernel: one work item per output element ----
    def im2col(self, px, c0, patch, ldo, n_img, img_cstride, out):
        m = self.mut
        B, C, H, W = px.shape
        gh, gw = H // patch, W // patch
        if m == "im2col_gh_gw":
            gh, gw = gw, gh
        total, kreal = B * n_img * gh * gw * ldo, 3 * patch * patch
        idx = torch.arange(total)
        k, r = idx % ldo, idx // ldo
        c, py, pxx = k // (patch * patch), (k // patch) % patch, k % patch
        if m == "im2col_py_px":
            py, pxx = pxx, py
        gx, gy, bi = r % gw, (r // gw) % gh, r // (gw * gh)
        b, img = bi // n_img, bi % n_img
        ch = c0 + (0 if m == "im2col_no_cstride" else img * img_cstride) + c
        src = ((b * C + ch) * H + gy * patch + py) * W + gx * patch + pxx
        flat = px.flatten().view(torch.int16)
        v = torch.where(k < kreal, flat[src.clamp(0, flat.numel() - 1)], torch.zeros((), dtype=torch.int16))
        written = torch.ones(total, dtype=torch.bool)
        if m == "im2col_stale_pad":
            written &= k < kreal
        if m == "im2col_one_trip":
            written &= idx < self.cap
        buf = out.buf.clone()
        region = buf.view(torch.int16)[out.pad:out.pad + out.n]
        region[written] = v[written]
        return buf

    # ---- image_prep_kernel: one work item per output pixel; frames addressed as the kernel does, from the base of the allocation ----
    def image_prep(self, frames, n, crop, crop_scale, out_size):
        m = self.mut
        _, H, W, _ = frames.shape
        flat = frames.numpy().reshape(-1)
        o = out_size
        if crop:
            side = np.clip(np.sqrt(F32(crop_scale)), F32(0), F32(1)).astype(F32)
            o1 = ((F32(1) - side) / F32(2)).astype(F32)
            o2 = (o1 + side).astype(F32)
            span = (o2 - o1).astype(F32)
            ystep, xstep = (span * F32(H - 1) / F32(o - 1)).astype(F32), (span * F32(W - 1) / F32(o - 1)).astype(F32)
            ybase, xbase = (o1 * F32(H - 1)).astype(F32), (o1 * F32(W - 1)).astype(F32)
            if m == "prep_xy_steps":
                ystep, xstep = xstep, ystep
            ar = np.arange(o, dtype=F32)
            ys, xs = (ybase + (ar * ystep).astype(F32)).astype(F32), (xbase + (ar * xstep).astype(F32)).astype(F32)
            outside = ((ys < 0) | (ys > F32(H - 1)))[:, None] | ((xs < 0) | (xs > F32(W - 1)))[None, :]
            if m == "prep_no_extrapolation":
                outside[:] = False
            fy, fx = np.floor(ys), np.floor(xs)
            y0, x0 = fy.astype(np.int64), fx.astype(np.int64)
            y1, x1 = (fy if m == "prep_floor_bottom" else np.ceil(ys)).astype(np.int64), np.ceil(xs).astype(np.int64)
            wy, wx = (ys - fy).astype(F32)[None, :, None, None], (xs - fx).astype(F32)[None, None, :, None]
            base = (np.arange(n, dtype=np.int64) * H * W * 3)[:, None, None, None]
            ch = np.arange(3, dtype=np.int64)[None, None, None, :]

            def tap(y, x):      # no load is issued for a pixel outside the image: its address is never formed
                a = base + ((y[:, None] * W + x[None, :]) * 3)[None, :, :, None] + ch
                a = np.where(outside[None, :, :, None], 0, a)
                return flat[np.clip(a, 0, flat.size - 1)].astype(F32) * (F32(1) / F32(255))
            tl, tr, bl, br = tap(y0, x0), tap(y0, x1), tap(y1, x0), tap(y1, x1)
            top = (tl + ((tr - tl).astype(F32) * wx).astype(F32)).astype(F32)
            bot = (bl + ((br - bl).astype(F32) * wx).astype(F32)).astype(F32)
            v = (top + ((bot - top).astype(F32) * wy).astype(F32)).astype(F32)
            scaled = (np.clip(v, F32(0), F32(1)) * F32(255.5)).astype(F32)
            q = (np.rint(scaled) if m == "prep_round" else scaled).astype(np.uint8)
            q = np.where(outside[None, :, :, None], np.uint8(0), q)
        else:
            q = frames[:n].numpy()
        x = torch.from_numpy(q.astype(F32) / F32(255)).permute(0, 3, 1, 2)                                  # [n, 3, o, o]
        mean, std = torch.tensor(R.IMAGE_MEAN, dtype=torch.float32), torch.tensor(R.IMAGE_STD, dtype=torch.float32)
        if m == "prep_mean_std_sets":
            mean, std = torch.cat([mean[3:], mean[:3]]), torch.cat([std[3:], std[:3]])
        full = ((torch.cat([x, x], 1) - mean[None, :, None, None]) / std[None, :, None, None]).to(BF)      # [n, 6, o, o]
        if m == "prep_one_trip":
            done = (torch.arange(n * o * o) < self.cap).view(n, 1, o, o)
            full = torch.where(done, full, R._sent(full.shape))
        return full.reshape(1, 6 * n, o, o)

    # ---- assemble_kernel: one workgroup per output row (b, s) ----
    def assemble(self, ids, labels, table, patches, noisy, A, out, apos):
        m = self.mut
        (B, L), (V, D), P = ids.shape, table.shape, patches.shape[1]
        S = P + L
        lab, idl = labels.tolist(), ids.tolist()
        ob, pb = out.buf.clone(), apos.buf.clone()
        for b in range(B):
            for s in range(S):
                if 1 <= s <= P or (m == "asm_s0_patches" and s == 0):
                    row = patches[b, max(s - 1, 0)]
                else:
                    i = 0 if s == 0 else s - P
                    cum = slot = is_action = 0
                    for j in range(i + 1):
                        cum += lab[b][j] != R.IGNORE
                        act = int(cum >= 1 and lab[b][j] > R.ACTION_BEGIN)
                        if j < i:
                            slot += int(lab[b][j] != R.IGNORE) if m == "asm_slot_all_labels" else act
                        else:
                            is_action = act
                    if is_action and (slot < A or m == "asm_pos_unbounded"):
                        p = apos.pad + b * A + slot
                        if p < pb.numel():
                            pb[p] = b * S + P + i - 1 + (1 if m == "asm_pos_plus_one" else 0)
                    if is_action:
                        row = noisy[b, slot] if noisy is not None and slot < A else torch.zeros(D, dtype=BF)
                    else:
                        t = idl[b][i] if m == "asm_no_clamp" else min(max(idl[b][i], 0), V - 1)
                        row = _flat_take(table.buf, table.pad + t * D, D, float("nan"))
                ncol = min(D, 2048) if m == "asm_2048_columns" else D
                o0 = out.pad + (b * S + s) * D
                ob[o0:o0 + ncol] = row[:ncol]
        return ob, pb

    # ---- language_average_kernel (lens None) and language_average_ragged_kernel ----
    def language_average(self, ids, labels, B, lens, table, out):
        m = self.mut
        L, (V, D) = ids.shape[1], table.shape
        fi, fl = ids.flatten().tolist(), labels.flatten().tolist()
        text = (lambda v: v < R.ACTION_BEGIN) if m == "lang_less_than" else (lambda v: v <= R.ACTION_BEGIN)
        ob = out.buf.clone()
        for b in range(B):
            n = L if lens is None else int(lens[b])
            if lens is not None and m != "lang_lens_unclamped":
                n = min(max(n, 0), L)
            s, cnt = torch.zeros(D), 0
            for i in range(n):
                p = b * L + i
                if p < len(fl) and text(fl[p]):
                    s = s + _flat_take(table.buf, table.pad + min(max(fi[p], 0), V - 1) * D, D, float("nan")).float()
                    cnt += 1
            if m == "lang_count_padding" and lens is not None:
                cnt += sum(text(fl[b * L + i]) for i in range(max(n, 0), L))
            den = L if m == "lang_divide_by_L" else max(cnt, 1)
            ob[out.pad + b * D:out.pad + (b + 1) * D] = (s / torch.tensor(float(den))).to(BF)
        return ob

    # ---- transpose_batched_kernel: one block per 64 x 64 tile of any entry ----
    def transpose_batched(self, pairs):
        m = self.mut
        starts = [0]
        for src, _ in pairs:
            starts.append(starts[-1] + -(-src.rows // 64) * -(-src.cols // 64))
        bufs = [dst.buf.clone() for _, dst in pairs]
        for blk in range(starts[-1]):
            lo, hi = 0, len(pairs) - 1
            while lo < hi:
                mid = (lo + hi + 1) >> 1
                if (starts[mid] < blk) if m == "tr_lookup_boundary" else (starts[mid] <= blk):
                    lo = mid
                else:
                    hi = mid - 1
            src, dst = pairs[lo]
            rows, cols = src.rows, src.cols
            t = blk - starts[lo]
            tiles_x = -(-(rows if m == "tr_tiles_x_rows" else cols) // 64)
            r0, c0 = (t // tiles_x) * 64, (t % tiles_x) * 64
            rr, cc = min(64, rows - r0), min(64, cols - c0)
            tile = torch.zeros((64, 64), dtype=BF)
            if rr > 0 and cc > 0:
                tile[:rr, :cc] = src.view[r0:r0 + rr, c0:c0 + cc]
            if m == "tr_edge_tiles_full":
                flat, ld = bufs[lo].view(-1), bufs[lo].shape[1]
                for c in range(64):
                    p = (dst.r0 + c0 + c) * ld + dst.c0 + r0
                    k = max(0, min(64, flat.numel() - p))
                    flat[p:p + k] = tile[:k, c]
            elif rr > 0 and cc > 0:
                bufs[lo][dst.r0 + c0:dst.r0 + c0 + cc, dst.c0 + r0:dst.c0 + r0 + rr] = tile[:rr, :cc].T
        return bufs

    # ---- row_sumsq_kernel: one wave per row, lane j owns slots j, j + 64, ... ----
    def row_sumsq(self, src, dim, out):
        m = self.mut
        rows, ld, slots = src.rows, src.buf.shape[1], dim // 64
        flat = src.buf.flatten()
        ob = out.buf.clone()
        stride = dim if m == "sumsq_ld_is_dim" else ld
        for r in range(-(-rows // 4) * 4 if m == "sumsq_rows_unbounded" else rows):
            seg = _flat_take(flat, src.r0 * ld + src.c0 + r * stride, dim, float("nan")).double().view(slots, 64).pow(2).sum(-1).float()
            live = min(slots, 64) if m == "sumsq_first_64_slots" else slots
            p = out.pad + r * slots
            k = max(0, min(live, ob.numel() - p))
            ob[p:p + k] = seg[:k]
        return ob


SUITES = {
    "im2col": lambda f, K: R.suite_im2col(f, K, cap=K.cap),
    "image_prep": lambda f, K: R.suite_image_prep(f, K, cap=K.cap),
    "assemble": lambda f, K: R.suite_assemble(f, K),
    "language_average": lambda f, K: R.suite_language_average(f, K),
    "transpose_batched": lambda f, K: R.suite_transpose_batched(f, K),
    "row_sumsq": lambda f, K: R.suite_row_sumsq(f, K),
}
NO_WRAP = {
    "im2col": lambda f, K: R.suite_im2col(f, K, wrap=None),
    "image_prep": lambda f, K: R.suite_image_prep(f, K, wrap=()),
}


@pytest.mark.parametrize("suite", list(SUITES))
def test_emulation_passes_every_check(suite):
    fails = R.Failures()
    SUITES[suite](fails, Emulated())
    fails.done()


# mutation -> (what is planted, its kernel, the suite run that must reject it, a phrase of each check meant to catch it: all must have failed)
MUTATIONS = {
    "im2col_no_cstride": ("img_cstride ignored: image 1 reads image 0's channels", "im2col", NO_WRAP["im2col"], ("n_img 2 cstride 6 28x42", "n_img 3 cstride 3")),
    "im2col_gh_gw": ("gh and gw swapped", "im2col", NO_WRAP["im2col"], ("28x42", "32x16")),
    "im2col_py_px": ("py and px swapped", "im2col", NO_WRAP["im2col"], ("14x14 patch 14 ldo 588", "patch 16")),
    "im2col_stale_pad": ("pad columns left as they were", "im2col", NO_WRAP["im2col"], ("ldo 592", "ldo 776")),
    "im2col_one_trip": ("the grid-stride loop stops after one trip", "im2col", SUITES["im2col"], "224x224"),
    "prep_no_extrapolation": ("no range test on the sampling coordinate (the kernel as it was)", "image_prep", NO_WRAP["image_prep"],
                              ("480x480 -> 384 crop_scale 1.0", "100x100 -> 96 crop_scale 1.5", "30x30 -> 224", "30x100 -> 45")),
    "prep_floor_bottom": ("floor for the bottom row", "image_prep", NO_WRAP["image_prep"], ("224x224 -> 224 crop_scale 0.9", "2x2 -> 2")),
    "prep_xy_steps": ("x and y steps swapped", "image_prep", NO_WRAP["image_prep"], ("256x320", "30x100")),
    "prep_round": ("round instead of truncate at * 255.5", "image_prep", NO_WRAP["image_prep"], "224x224 -> 224 crop_scale 0.9"),
    "prep_one_trip": ("the grid-stride loop stops after one trip", "image_prep", SUITES["image_prep"], ("22 x 224x224 -> 224 crop_scale None", "22 x 224x224 -> 224 crop_scale 0.9")),
    "prep_mean_std_sets": ("the two mean / std sets swapped", "image_prep", NO_WRAP["image_prep"], ("crop_scale None", "2x2 -> 2")),
    "asm_slot_all_labels": ("slot counted from all non-ignored labels", "assemble", SUITES["assemble"], "'other labels' noisy True: out"),
    "asm_pos_unbounded": ("action_pos written for slot >= A", "assemble", SUITES["assemble"], "'A + 2' noisy False: action_pos"),
    "asm_pos_plus_one": ("action_pos off by one row", "assemble", SUITES["assemble"], ("'exactly A' noisy False: action_pos", "'at index 0' noisy True: action_pos")),
    "asm_no_clamp": ("ids not clamped: reads a NaN guard row", "assemble", SUITES["assemble"], "'edge ids' noisy False: out"),
    "asm_2048_columns": ("only the first 2048 columns written", "assemble", SUITES["assemble"], "D 2056"),
    "asm_s0_patches": ("the s = 0 row taken from the patches", "assemble", SUITES["assemble"], ("L 1 P 1 D 8", "D 264")),
    "lang_less_than": ("< for <= at action_token_begin", "language_average", SUITES["language_average"], ("plain D 8", "ragged D 264")),
    "lang_count_padding": ("the count includes the padding", "language_average", SUITES["language_average"], "ragged D 8 lens (4, 5, 6, 7, 3)"),
    "lang_lens_unclamped": ("lens not clamped", "language_average", SUITES["language_average"], ("lens (1, 9, 0, -3, 14)", "lens (9, 0, -3, 14, 1)")),
    "lang_divide_by_L": ("divide by L", "language_average", SUITES["language_average"], ("plain D 520", "ragged D 8")),
    "tr_lookup_boundary": ("the entry lookup off by one at a boundary tile", "transpose_batched", SUITES["transpose_batched"], ("nine entries: entry 64x64", "reversed: entry 1x1")),
    "tr_tiles_x_rows": ("tiles_x computed from rows", "transpose_batched", SUITES["transpose_batched"], ("entry 63x65", "entry 96x300", "one entry")),
    "tr_edge_tiles_full": ("edge tiles written in full", "transpose_batched", SUITES["transpose_batched"], ("entry 1x1", "entry 65x63")),
    "sumsq_ld_is_dim": ("ld taken as dim", "row_sumsq", SUITES["row_sumsq"], ("ld 136", "ld 4168")),
    "sumsq_first_64_slots": ("slots beyond the first 64 dropped", "row_sumsq", SUITES["row_sumsq"], "dim 4160"),
    "sumsq_rows_unbounded": ("rows >= rows written", "row_sumsq", SUITES["row_sumsq"], ("rows 1 dim 64", "rows 5", "rows 7")),
}


# ---- what covered these kernels before: the same inputs and the same assertions, on whatever K computes ---------------------------------------
def _rnd(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(BF)


def _plain(t):
    """A contiguous 2-D tensor as an Embedded without guards."""
    return R.Embedded(t, 0, 0, t.shape[0], t.shape[1])


def old_im2col(K):
    """test_vision_front_end_glue's im2col lines."""
    g = R.rng(4)
    px = _rnd(g, 2, 12, 56, 56)
    out = R.Slab(BF, (2 * 16, 592))
    cols = K.im2col(px, 3, 14, 592, 1, 6, out)[out.pad:out.pad + out.n].view(32, 592)
    ref = torch.nn.functional.unfold(px[:, 3:6].float(), kernel_size=14, stride=14).transpose(1, 2).reshape(32, 588)
    return torch.equal(cols[:, :588].float(), ref) and bool(cols[:, 588:].abs().max() == 0)


def old_image_prep(K):
    """test_image_prep_bit_exact_vs_oracle: three frames, 224x224 and 256x320 with the crop at 0.9, 224x224 without."""
    for (H, W), crop in (((224, 224), True), ((256, 320), True), ((224, 224), False)):
        r = np.random.default_rng(H * 7 + W + int(crop))
        imgs = r.integers(0, 256, (4, H, W, 3), dtype=np.uint8)
        imgs[0, :8] = 255
        imgs[1, :, :8] = 0
        frames = torch.from_numpy(imgs)
        ref, _ = R.image_prep_ref(frames, 3, 0.9 if crop else None, 224)
        if not torch.equal(K.image_prep(frames, 3, crop, 0.9, 224), ref):
            return False
    return True


def old_assemble(K):
    """test_assemble_and_gather's assemble lines: one ragged batch with exactly A action tokens, D = 64."""
    g = R.rng(6)
    B, Tp, A, D, P, V = 3, 6, 14, 64, 10, 32064
    L = Tp + A + 1 + 2
    ids = torch.randint(3, 31000, (B, L), generator=g)
    labels = torch.full((B, L), -100, dtype=torch.long)
    for b_, tp in enumerate([Tp, Tp + 2, Tp - 1]):
        ids[b_, tp:tp + A] = torch.randint(31744, 32000, (A,), generator=g)
        ids[b_, tp + A] = 2
        ids[b_, tp + A + 1:] = 32000
        labels[b_, tp:tp + A + 1] = ids[b_, tp:tp + A + 1]
    table = R.Slab(BF, (V, D), fill="nan", pad=4 * D, src=_rnd(g, V, D))
    patches, noisy = _rnd(g, B, P, D), _rnd(g, B, A, D)
    amask = ((labels != -100).cumsum(1) >= 1) & (labels > 31743)
    emb = table.view[ids]
    for use_noisy in (False, True):
        e = emb.clone()
        if use_noisy:
            for b_ in range(B):
                e[b_, amask[b_]] = noisy[b_]
        else:
            e = e * (~amask)[..., None]
        ref = torch.cat([e[:, :1], patches, e[:, 1:]], 1)
        out, apos = R.Slab(BF, (B, P + L, D)), R.Slab(torch.int32, (B, A))
        apos.view.fill_(-1)
        ob, pb = K.assemble(ids, labels, table, patches, noisy if use_noisy else None, A, out, apos)
        if not torch.equal(ob[out.pad:out.pad + out.n].view(ref.shape), ref):
            return False
        got = pb[apos.pad:apos.pad + apos.n].view(B, A)
        if not all(torch.equal(got[b_].long(), b_ * (P + L) + P + torch.where(amask[b_])[0] - 1) for b_ in range(B)):
            return False
    return True


def old_ragged(K):
    """tests/test_ragged_average_gpu.py, both tests."""
    IGN, STOP, ACTION, B, L, D, VOCAB, PAD = -100, 2, 31744 + 5, 3, 24, 64, 512, 511
    g = torch.Generator().manual_seed(11)
    rows = torch.randn(VOCAB, D, generator=g).to(BF)
    rows[PAD] = 1e3
    table = R.Slab(BF, (VOCAB, D), fill="nan", pad=4 * D, src=rows)
    ids0 = torch.randint(1, 500, (B, L), generator=g)
    labels0 = torch.full((B, L), IGN, dtype=torch.int64)
    labels0[0, 16:23], labels0[0, 23] = ACTION, STOP
    labels0[1, 10:17] = ACTION
    labels0[2, 5:8], labels0[2, 8] = ACTION, STOP
    guard = lambda n: (torch.full((1, n), PAD), torch.full((1, n), IGN))  # noqa: E731
    for lens in ((24, 17, 9), (1, 1, 1)):
        ids, labels = ids0.clone(), labels0.clone()
        for b, n in enumerate(lens):
            ids[b, n:], labels[b, n:] = PAD, IGN
        out = R.Slab(BF, (8, D))
        out.view.zero_()
        gi, gl = guard(L)
        got = K.language_average(torch.cat([ids, gi]), torch.cat([labels, gl]), B, torch.tensor(lens, dtype=torch.int32), table, out)[out.pad:out.pad + out.n].view(8, D)
        if not torch.equal(got[B:], torch.zeros_like(got[B:])):
            return False
        for b, n in enumerate(lens):
            alone = R.Slab(BF, (1, D))
            gi, gl = guard(n)
            one = K.language_average(torch.cat([ids[b:b + 1, :n], gi]), torch.cat([labels[b:b + 1, :n], gl]), 1, None, table, alone)[alone.pad:alone.pad + D]
            keep = labels[b, :n] <= 31743
            s = torch.zeros(D)
            for i in torch.nonzero(keep).flatten().tolist():
                s = s + rows[ids[b, i]].float()
            ref = s / float(keep.sum())
            if not (torch.equal(got[b].view(torch.int16), one.view(torch.int16)) and torch.allclose(got[b].float(), ref, rtol=2.0 ** -8, atol=1e-6)
                    and got[b].float().abs().max().item() < 10.0):
                return False
    return True


def old_transpose(K):
    """test_gemm_tn_grouped_and_block_diagonal's batched transposes: three contiguous entries, the logical region compared."""
    g = R.rng(21)
    srcs = [_rnd(g, 96, 300), _rnd(g, 520, 32), _rnd(g, 64, 64)]
    dsts = [torch.zeros((s.shape[1], s.shape[0]), dtype=BF) for s in srcs]
    got = K.transpose_batched([(_plain(s), _plain(d)) for s, d in zip(srcs, dsts)])
    return all(torch.equal(d, s.T.contiguous()) for s, d in zip(srcs, got))


def old_row_sumsq(K):
    """test_gemm_rmsnorm_fold's row_sumsq line at the smallest and the largest of its shapes (rows % 4 == 0, ld == dim <= 4096 in all of them)."""
    g = R.rng(608)
    for rows, dim in ((300, 512), (608, 4096)):
        x = _rnd(g, rows, dim)
        out = R.Slab(torch.float32, (rows, dim // 64))
        got = K.row_sumsq(_plain(x), dim, out)[out.pad:out.pad + out.n].view(rows, dim // 64)
        ref = x.float().view(rows, dim // 64, 64).pow(2).sum(-1)
        if not torch.allclose(got, ref, rtol=1e-5, atol=1e-5 * ref.abs().max().item()):
            return False
    return True


OLD_TESTS = {"im2col": old_im2col, "image_prep": old_image_prep, "assemble": old_assemble, "language_average": old_ragged, "transpose_batched": old_transpose,
             "row_sumsq": old_row_sumsq}
# Filled from a run of this file: the planted bugs the earlier tests ACCEPT, because their one shape does not reach them -- n_img = 1, square
# images below one trip of the loop, crop_scale 0.9 only, exactly A action tokens after a prompt of ignored labels with ids inside the
# vocabulary and D = 64, lens inside [1, L] with no label at the threshold, rows % 4 == 0 with ld == dim <= 4096.
OLD_TESTS_ACCEPT = {"im2col_no_cstride", "im2col_gh_gw", "im2col_one_trip", "prep_no_extrapolation", "prep_one_trip", "asm_slot_all_labels", "asm_pos_unbounded",
                    "asm_no_clamp", "asm_2048_columns", "lang_less_than", "lang_lens_unclamped", "sumsq_ld_is_dim", "sumsq_first_64_slots", "sumsq_rows_unbounded"}


@pytest.mark.parametrize("kernel", list(OLD_TESTS))
def test_the_earlier_tests_accept_the_correct_restatement(kernel):
    assert OLD_TESTS[kernel](Emulated(cap=R.GRID_CAP_ITEMS))


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_planted_bug_is_rejected_and_what_the_earlier_tests_say(name):
    what, kernel, run, phrase = MUTATIONS[name]
    fails = R.Failures()
    run(fails, Emulated(name))
    assert fails, f"{name} ({what}): not rejected"
    for ph in ((phrase,) if isinstance(phrase, str) else phrase):
        assert any(ph in m for m in fails), f"{name}: rejected, but not by the check meant to catch it ({ph!r}):\n" + "\n".join(fails[:5])
    accepted = OLD_TESTS[kernel](Emulated(name, cap=R.GRID_CAP_ITEMS))          # the earlier tests ran the real kernels: the real cap
    print(f"{name}: {what}\n    new suite: rejected ({len(fails)} failures; first: {fails[0][:160]})\n    earlier tests: {'ACCEPT' if accepted else 'reject'}")
    assert accepted == (name in OLD_TESTS_ACCEPT), f"{name}: the earlier tests {'accept' if accepted else 'reject'} it"


def test_the_kernel_as_it_was_fails_at_the_overshoot_shapes_and_nowhere_else():
    """image_prep_kernel without the range test: with the guard frame behind the frames it reads defined memory, and differs from the reference
    in every overshoot case (four shapes, crop_scale 1.0 and 1.5) and in no other case, the two grid-stride cases included."""
    fails = R.Failures()
    R.suite_image_prep(fails, Emulated("prep_no_extrapolation"), cap=4096)
    want = {f"image_prep {n} x {H}x{W} -> {o} crop_scale {s}" for H, W, o, s, n in R.PREP_OVERSHOOT}
    assert len(want) == 8 and {m.split(":")[0] for m in fails} == want, "\n".join(fails)


OVERSHOOT = ((480, 480, 384), (100, 100, 96), (30, 30, 224), (30, 100, 45))


@pytest.mark.parametrize("crop_scale", [1.0, 1.5, 0.9])
def test_both_oracles_mark_the_same_pixels_as_outside_the_image(crop_scale):
    """On the box (o1, o1, o2, o2) of the center crop, vla_oracle.crop_and_resize_center and data_oracle.crop_and_resize agree on which output
    pixels lie outside the image (a white frame: a pixel is black exactly where the extrapolation value was taken); at the overshoot shapes
    with the box clipped to the whole image that is the last row and / or column, at 0.9 nothing."""
    from oracle import data_oracle as do
    from oracle import vla_oracle as vo

    side = np.clip(np.sqrt(F32(crop_scale)), F32(0), F32(1)).astype(F32)
    o1 = ((F32(1) - side) / F32(2)).astype(F32)
    o2 = (o1 + side).astype(F32)
    for H, W, out in OVERSHOOT:
        white = np.full((H, W, 3), 255, dtype=np.uint8)
        a = vo.crop_and_resize_center(white, crop_scale, out) == 0
        b = do.crop_and_resize(white.astype(F32) * F32(1.0 / 255.0), (o1, o1, o2, o2), out) == 0
        assert np.array_equal(a, b), f"{H}x{W} -> {out} at {crop_scale}: {int((a != b).sum())} pixels marked differently"
        inner = a[:-1, :-1]
        assert not inner.any() and (a.any() == (crop_scale >= 1.0)), f"{H}x{W} -> {out} at {crop_scale}: {int(a.sum())} pixels outside"


def test_center_crop_image_is_the_oracle_crop():
    """The host mirror of the kernel's crop returns the oracle's pixels, at an overshoot shape (where both used to raise IndexError) and at 0.9."""
    import importlib

    ip = importlib.import_module("openvla-oft_amd.image_prep")
    from oracle import vla_oracle as vo

    r = np.random.default_rng(5)
    for H, W, out, scale in ((30, 100, 45, 1.0), (100, 100, 96, 1.5), (224, 224, 224, 0.9)):
        im = r.integers(1, 256, (H, W, 3), dtype=np.uint8)
        got = ip.center_crop_image(im, scale, out)
        assert np.array_equal(got, vo.crop_and_resize_center(im, scale, out))
        assert (got[-1] == 0).all() == (scale >= 1.0)
