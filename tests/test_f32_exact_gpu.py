"""Every op of the f32 parity mode (csrc/kernels_f32.hip, Network::run_f32) against tests/exact_ref_f32.py, element by element.

The mode's claim -- every convolution output is the correctly rounded value of its exact sum, everything behind that one
rounding is plain f32 in a fixed order -- is held per op at four geometries, each named for an edge in conv_f32_kernel's
indexing (64 x 64 output tiles, K steps of 16):

  32x32   n=4   M = 256, 64, 16, 4: whole tiles down to a 4-row tile; the 1x1 -> 2x2 up-2 residual
  96x64   n=3   M = 1152, 288 (tail 32), 72, 18; a 3-wide map from a stride-2 conv of a 6-wide one
  160x96  n=1   M = 960, 240, 60, 15; the odd 5x3 map under the up-2 residual of a 10x6 one
  320x256 n=2   M = 10 240: many tiles per N column

Every op runs alone (debug_run(n, i, i)) on two input sets (tests/f32_exact_cases.py):
- random: the synthetic weights (not bf16 values) and full-mantissa operands.  Every decided element must hold the one legal
  value, every undecided one must lie between its two, and the undecided share of every output stays <= 1 %;
- dyadic: every sum is exact in any order, so every element is decided: borders and tile tails are held bit for bit.
Before the launch every channel the op writes holds NaN bits: every written element must be overwritten, every byte of the
output tensor outside the op's channels and every operand the op only reads must come back unchanged.  The second convolution
of a back-to-back op is judged from the device's own stored first output.  The soft-maxed score channels of the heads follow
exact_ref.check_f32's ulp rule, from the f32 logit difference the device forms (exact_ref_f32.Out); the box and landmark
channels are exact.

Printed per geometry: cases, elements, undecided elements, and among those the ones the device did not round to the epilogue of
float32(v64) -- the measured size of "summation-order noise straddles an f32 rounding boundary" (profiles/f32_exact_sweep.txt)."""
import numpy as np
import pytest
import torch

import exact_ref_f32
import f32_exact_cases
import torch_ref
from test_conv_exact_gpu import NAN_F32, _dyadic_weights, _first_bad

pytestmark = pytest.mark.gpu

GEOMETRIES = [(32, 32, 4), (96, 64, 3), (160, 96, 1), (320, 256, 2)]   # (image w, image h, images)
assert all(w % 32 == 0 and h % 32 == 0 for w, h, _ in GEOMETRIES)   # the graph's own requirement


class SweepF32:
    def __init__(self, det, g, geo, n):
        self.det, self.g, self.geo, self.n = det, g, geo, n
        self.fail = []
        self.cases = self.elements = self.undecided = self.off = 0
        self.worst = 0.0

    def _dev(self, t, x):
        td = self.g.tensors[t]
        return torch_ref.nchw_to_dev(x, is_f32=self.det.debug_dtype(td) == np.float32, channels=td.channels)

    def run_set(self, dyadic, seed):
        g = self.g
        ref = exact_ref_f32.ExactRefF32(g, self.det)
        ref.radius, ref.exact = not dyadic, dyadic
        rng = np.random.default_rng(seed)
        for i, o in enumerate(g.ops):
            tens = f32_exact_cases.inputs(rng, g, o, self.n, dyadic)
            with torch.no_grad():
                want = ref.run_op(i, tens)
            self.cases += 1
            self._run_case(ref, i, tens, want, "dyadic" if dyadic else "random", 0.0 if dyadic else 0.01)

    def _run_case(self, ref, i, tens, want, tag, cap):
        det, g, n = self.det, self.g, self.n
        o = g.ops[i]
        what = "op %d (%s, kind %d) at %s n = %d, %s set" % (i, g.layers[o.layer].name.decode(), o.kind, self.geo, n, tag)
        sent = {t: self._dev(t, x) for t, x in tens.items()}
        for t, a in sent.items():
            det.debug_write(t, a)
        outs = [t for t in (o.out, o.out2, o.outf, o.out_b) if t >= 0]
        prior = {}
        for t in outs:
            td = g.tensors[t]
            a = sent[t].copy() if t in sent else np.zeros((n, td.height, td.width, td.channels), np.float32)
            written = want[t].dst if (t in want and want[t].dst is not None) else np.arange(td.channels_logical)
            if t == o.in_:
                assert not set(written) & set(range(o.x_coff, o.x_coff + g.layers[o.layer].cin)), "in-place op overwrites its input"
            a.view(np.uint32)[..., written] = NAN_F32
            det.debug_write(t, a)
            prior[t] = (a, written)
        det.debug_run(n, i, i)
        for t, a in sent.items():
            if t not in prior and not np.array_equal(det.debug_read(t, n, g.tensors[t]).view(np.uint8), a.view(np.uint8)):
                self.fail.append("%s tensor %d: the op changed an operand it only reads" % (what, t))
        for t in outs:
            td = g.tensors[t]
            got = det.debug_read(t, n, td)
            a, written = prior[t]
            keep = np.setdiff1d(np.arange(td.channels), written)
            if not np.array_equal(np.ascontiguousarray(got[..., keep]).view(np.uint8), np.ascontiguousarray(a[..., keep]).view(np.uint8)):
                self.fail.append("%s tensor %d: bytes outside the op's channels changed" % (what, t))
            g32 = np.ascontiguousarray(got[..., written].transpose(0, 3, 1, 2))
            if t in want:
                w = want[t]
            else:   # out_b: computed from the device's own stored first output
                src = o.out if o.out >= 0 else o.out2
                first = det.debug_read(src, n, g.tensors[src])[..., :g.tensors[src].channels_logical]
                if bool(np.isnan(first).any()):   # reported with tensor src itself; the reference cannot start from NaN
                    self.fail.append("%s tensor %d: not checked, the stored tensor %d it is computed from holds NaN" % (what, t, src))
                    continue
                with torch.no_grad():
                    w = ref.second(i, torch.from_numpy(np.ascontiguousarray(first.transpose(0, 3, 1, 2))))
            bad, und, off = exact_ref_f32.check(g32, w)
            self.elements += bad.size
            self.undecided += int(und.sum())
            self.off += int(off.sum())
            share = float(w.und.mean())
            self.worst = max(self.worst, share)
            if share > cap:
                self.fail.append("%s tensor %d: %.3f %% of the outputs undecided (cap %.0f %%)" % (what, t, 100 * share, 100 * cap))
            left = int(np.isnan(g32).sum())
            if left:
                self.fail.append("%s tensor %d: %d / %d written elements still hold NaN" % (what, t, left, g32.size))
            if bool(bad.any()):
                p = _first_bad(torch.from_numpy(bad))
                b0 = p[0]
                score = w.softmax and b0[1] < 4   # judged by exact_ref.check_f32 from the ends of D = float32(bg - fg)
                ends = w.score if score else w
                at = (b0[0], b0[1] % 2, b0[2], b0[3]) if score else b0
                self.fail.append("%s tensor %d: %d / %d elements wrong, first at (n, c, y, x) %s: got %r, %s [%r, %r], v64 %r" % (
                    what, t, int(bad.sum()), bad.size, p, float(g32[b0]), "softmax of the logit difference in" if score else "legal",
                    float(ends.lo[at]), float(ends.hi[at]), float(w.v64[b0])))


@pytest.mark.parametrize("geom", GEOMETRIES, ids=["%dx%d-n%d" % g for g in GEOMETRIES])
def test_every_f32_op_matches_the_exact_reference(rfd, geom):
    w, h, n = geom
    det = rfd.RetinaFaceDetection(image_size=(w, h), max_batch_size=n, max_det=16, precision=rfd.PRECISION_F32)
    try:
        det.init_synthetic_weights(1234)
        g = rfd.Graph(rfd.BACKBONE_R50, w, h)
        for i, L in enumerate(g.layers):
            wl, _ = det.get_layer(i, L)
            assert np.any(wl.view(np.uint32) & 0xFFFF), "layer %d: the synthetic weights are bf16 values" % i
        sw = SweepF32(det, g, "r50 %dx%d" % (w, h), n)
        sw.run_set(dyadic=False, seed=31)
        rnd = (sw.elements, sw.undecided, sw.off, sw.worst)
        _dyadic_weights(det, g, np.random.default_rng(32))
        sw.run_set(dyadic=True, seed=33)
        print("\nf32 exact sweep r50 %dx%d n=%d: %d cases, %d failures; random set: %d elements, %d undecided (worst output %.3f %%), "
              "%d of them not the rounding of v64; dyadic set: %d elements, %d undecided" % (
                  w, h, n, sw.cases, len(sw.fail), rnd[0], rnd[1], 100 * rnd[3], rnd[2], sw.elements - rnd[0], sw.undecided - rnd[1]))
        assert not sw.fail, "\n".join(sw.fail[:12]) + ("\n... %d more" % (len(sw.fail) - 12) if len(sw.fail) > 12 else "")
        assert sw.cases == 2 * len(g.ops) and sw.undecided == rnd[1]
    finally:
        det.close()


def test_tensor_hook_moves_f32_intermediates(rfd):
    """rfd_debug_tensor_io in the f32 parity mode: an intermediate tensor goes in and comes back as n * C*H*W floats, beside (not
    over) its neighbours; the network input stays the bf16 NHWC4 tensor; an array of the wrong element type is refused."""
    n = 2
    det = rfd.RetinaFaceDetection(image_size=(32, 32), max_batch_size=n, max_det=16, precision=rfd.PRECISION_F32)
    try:
        det.init_synthetic_weights(1)
        g = rfd.Graph(rfd.BACKBONE_R50, 32, 32)
        rng = np.random.default_rng(5)
        o = g.ops[1]
        sent = {}
        for t in (g.ops[0].in_, o.in_, o.out):
            td = g.tensors[t]
            dt = det.debug_dtype(td)
            assert dt == (np.uint16 if td.is_input else np.float32)
            a = rng.integers(0, 255, size=(n, td.height, td.width, td.channels)).astype(dt) if td.is_input else \
                rng.normal(size=(n, td.height, td.width, td.channels)).astype(np.float32)
            det.debug_write(t, a)
            sent[t] = a
        for t, a in sent.items():
            back = det.debug_read(t, n, g.tensors[t])
            assert back.dtype == a.dtype and np.array_equal(back.view(np.uint8), a.view(np.uint8)), t
        with pytest.raises(rfd.RfdError) as e:
            det.debug_write(o.in_, sent[o.in_].astype(np.uint16))
        assert e.value.status == rfd.RFD_ERR_INVALID_ARG
    finally:
        det.close()
