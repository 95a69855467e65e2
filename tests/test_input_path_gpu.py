"""The input-path kernels of csrc/elementwise.hip -- im2col, image_prep, assemble, the two language averages, the batched transpose, row_sumsq --
against the integer / float64 references of tests/input_path_reference.py: bit equality of whole allocations, outputs inside sentinel guards,
inputs inside NaN guards.  The suites (shapes, data, checks) are the ones tests/test_input_path_reference.py runs on a restatement of the
kernels with planted bugs; here `Real` hands them the real launches.
"""
import pytest
import torch

from tests import input_path_reference as R

pytestmark = pytest.mark.gpu
BF = torch.bfloat16


class Real:
    """The suites' K for the real library: CPU tensors in, launches through `ops` on `dev`, CPU tensors out.  Allocations keep their layout on
    the device (Slab.on / Embedded), so guards are guards there too."""

    def __init__(self, ops, dev):
        self.ops, self.dev = ops, dev

    def _emb(self, e):
        return R.Embedded(e.buf.to(self.dev), e.r0, e.c0, e.rows, e.cols)

    def im2col(self, px, c0, patch, ldo, n_img, img_cstride, out):
        # ops.im2col allocates its own output: the argument struct is filled here so that the output lies inside guards
        ops, p, o = self.ops, px.to(self.dev), out.on(self.dev)
        B, C, H, W = px.shape
        g = ops.STRUCTS["ovla_im2col_args"]()
        g.pixels, g.out, g.ldo, g.B, g.C_total, g.c0, g.H, g.W, g.patch = p.data_ptr(), o.view.data_ptr(), ldo, B, C, c0, H, W, patch
        g.n_img, g.img_cstride = n_img, img_cstride
        ops._lib.call("ovla_im2col", g, ops._stream())
        return o.buf.cpu()

    def image_prep(self, frames, n, crop, crop_scale, out_size):
        return self.ops.image_prep(frames.to(self.dev)[:n], crop=crop, crop_scale=crop_scale, out_size=out_size).cpu()

    def assemble(self, ids, labels, table, patches, noisy, A, out, apos):
        t, o, p = table.on(self.dev), out.on(self.dev), apos.on(self.dev)
        self.ops.assemble_multimodal(ids.to(self.dev), labels.to(self.dev), t.view, patches.to(self.dev), A=A, noisy=None if noisy is None else noisy.to(self.dev),
                                     out=o.view, action_pos=p.view)
        return o.buf.cpu(), p.buf.cpu()

    def language_average(self, ids, labels, B, lens, table, out):
        t, o = table.on(self.dev), out.on(self.dev)
        i, lab = ids.to(self.dev)[:B], labels.to(self.dev)[:B]
        if lens is None:
            self.ops.language_average(i, lab, t.view, o.view)
        else:
            self.ops.language_average_ragged(i, lab, lens.to(self.dev), t.view, o.view)
        return o.buf.cpu()

    def transpose_batched(self, pairs):
        on = [(self._emb(s), self._emb(d)) for s, d in pairs]
        self.ops.transpose_batched(self.ops.transpose_table([(s.view, d.view) for s, d in on], self.dev))
        return [d.buf.cpu() for _, d in on]

    def row_sumsq(self, src, dim, out):
        s, o = self._emb(src), out.on(self.dev)
        self.ops.row_sumsq(s.view, out=o.view)
        return o.buf.cpu()


def run(suite, ops, dev):
    fails = R.Failures()
    suite(fails, Real(ops, dev))
    fails.done()


def test_im2col_images_per_row_strides_patches_and_a_second_trip(ops, dev):
    """n_img 1 / 2 / 3 with img_cstride 6 / 3, c0 0 / 3, H != W both ways, patch 14 / 16, ldo == 3 patch^2 and beyond, random bit patterns with
    NaN in the channels not selected, the output inside sentinel guards; 4 x 2 images of 224 x 224 (1,212,416 work items)."""
    run(R.suite_im2col, ops, dev)


def test_image_prep_shapes_overshoot_and_a_second_trip(ops, dev):
    """The shapes the project runs; the four shapes at which the last sampling coordinate rounds above H - 1 with the box clipped to the whole
    image (crop_scale 1.0 and 1.5): TF's black pixel, no read past the frame; 2x2 -> 2; 22 frames (1,103,872 pixels), crop on and off."""
    run(R.suite_image_prep, ops, dev)


def test_assemble_action_slots_clamped_ids_and_wide_rows(ops, dev):
    """More, fewer and no action tokens than A, one at text index 0, counted labels that are no actions, ids -1 / vocab / 2^40, L = 1,
    D = 2056; with and without `noisy`; out and action_pos (pre-filled with -1) as whole allocations."""
    run(R.suite_assemble, ops, dev)


def test_language_average_exact_and_ragged_edges(ops, dev):
    """Integer table rows (exact sums): one / no / all text positions, a label at the threshold, clamped ids, lens in {1, L, 0, -3, L + 5}
    and inside the row with NaN rows behind it, D 8 / 264 / 520, out[B:] untouched."""
    run(R.suite_language_average, ops, dev)


def test_transpose_batched_mixed_entries_in_guards(ops, dev):
    """Nine entries from 1x1 to 520x32, single-tile next to many-tile, strided sources (NaN guards) and destinations (sentinel guards),
    forwards, reversed and one entry alone."""
    run(R.suite_transpose_batched, ops, dev)


def test_row_sumsq_exact(ops, dev):
    """rows % 4 != 0, ld > dim with NaN beyond dim, 65 slots (lane 0 runs its second), integer data: exact."""
    run(R.suite_row_sumsq, ops, dev)
