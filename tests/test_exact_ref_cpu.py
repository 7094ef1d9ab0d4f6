"""tests/exact_ref.py against torch_ref.TorchRef (torch-CPU f32) on small shapes, no GPU: every f32 result must lie in the
legal set the f64 reference computes, and on the dyadic data the f32 sums must be exact (torch f32 == f64, bit for bit).

Both statements are about f32 SUMS of the products, in some order.  torch's CPU convolution picks its algorithm by machine
(oneDNN, NNPACK: on some CPUs Winograd-style transforms, whose f32 results are no such sum), so these tests switch both off:
F.conv2d then runs as im2col + sgemm, an ordinary f32 dot product on every CPU."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_ref
import helpers
import torch_ref


class _Weights:
    """get_layer / get_affine / set_* of a detector context, host-side (the reference reads nothing else)."""

    def __init__(self, g, rng, dyadic):
        self.w, self.b, self.aff = [], [], []
        feeds = {o.layer for o in g.ops if o.kind in (3, 6)}   # the same data as test_conv_exact_gpu._dyadic_weights
        second = {o.layer_b for o in g.ops if o.kind == 6}
        for i, L in enumerate(g.layers):
            shape = (L.cout, L.kh, L.kw, L.cin)
            if dyadic:
                k = 2 if i in second else 8
                self.w.append((rng.integers(-k, k + 1, size=shape) * 2.0 ** -6).astype(np.float32))
                self.b.append((rng.integers(-64, 65, size=L.cout) * 2.0 ** -6 if L.kind == 3 else
                               rng.integers(-512, 513, size=L.cout) * 2.0 ** -10).astype(np.float32))
                s = rng.choice([1.0, -1.0] if i in feeds else [1.0, 0.5, 0.25, -0.5], size=L.cout)
                t = rng.integers(-16, 17, size=L.cout) * 2.0 ** -4
            else:
                fan = L.kh * L.kw * L.cin
                self.w.append(helpers.bf16_round(rng.normal(0, 1.4 / np.sqrt(fan), size=shape).astype(np.float32)))
                self.b.append(rng.normal(0, 0.1, size=L.cout).astype(np.float32))
                s = rng.uniform(-0.2, 1.5, size=L.cout)
                t = rng.normal(0, 0.2, size=L.cout)
            self.aff.append((s.astype(np.float32), t.astype(np.float32)))

    def get_layer(self, i, L):
        return self.w[i], self.b[i]

    def get_affine(self, i, cout):
        return self.aff[i]


def _inputs(rng, g, o, n, dyadic):
    def act(td, signed):
        shape = (n, td.channels_logical, td.height, td.width)
        if dyadic:
            return torch.from_numpy(rng.integers(-15 if signed else 0, 16, size=shape) * 2.0 ** -4).float()
        x = rng.normal(0, 1, size=shape).astype(np.float32)
        return torch.from_numpy(helpers.bf16_round(x if signed else np.maximum(x, 0)))
    tin = g.tensors[o.in_]
    tens = {}
    if o.kind in (0, 3, 5):
        x = rng.integers(0, 256, size=(n, 4, tin.height, tin.width)).astype(np.float32)
        x[:, 3] = 0
        tens[o.in_] = torch.from_numpy(x)
    else:
        tens[o.in_] = act(tin, o.in_affine >= 0)
    if o.in2 >= 0:
        tens[o.in2] = act(g.tensors[o.in2], False)
    if o.res >= 0:
        tens[o.res] = act(g.tensors[o.res], True)
    if o.out >= 0 and o.out != o.in_ and g.tensors[o.out].channels_logical != g.layers[o.layer].cout:
        tens[o.out] = act(g.tensors[o.out], False)
    return tens


def _got(tens, t, out):
    v = tens[t].double()
    return v[:, out.dst] if out.dst is not None else v


@pytest.fixture(autouse=True)
def _summing_f32_conv():
    saved = torch.backends.mkldnn.enabled, torch._C._get_nnpack_enabled()
    torch.backends.mkldnn.enabled = False
    torch.backends.nnpack.set_flags(False)
    try:
        yield
    finally:
        torch.backends.mkldnn.enabled = saved[0]
        torch.backends.nnpack.set_flags(saved[1])


@pytest.fixture(scope="module", params=["r50", "mnet025"])
def graph(request):
    import rfd_hip
    rfd_hip.load_library()
    bb = rfd_hip.BACKBONE_R50 if request.param == "r50" else rfd_hip.BACKBONE_MNET025
    return rfd_hip.Graph(bb, 64, 64)


def test_rne_bf16_rounds_ties_to_even():
    one = 1.0 + 2.0 ** -8   # half way between 1 and 1 + 2^-7: the even neighbour is 1
    x = torch.tensor([one, 1.0 + 3 * 2.0 ** -8, -one, 0.0, 1.0 + 2.0 ** -8 + 2.0 ** -40],
                     dtype=torch.float64)
    assert exact_ref.rne_bf16(x).tolist() == [1.0, 1.0 + 2.0 ** -6, -1.0, 0.0, 1.0 + 2.0 ** -7]
    assert exact_ref.bf16_ties(x) == (2, 1)
    rng = np.random.default_rng(3)
    f = (rng.normal(0, 1, 100000) * np.exp2(rng.integers(-20, 20, 100000))).astype(np.float32)
    f[:1000] = helpers.bf16_round(f[:1000]) * np.float32(1 + 2.0 ** -8)   # many exact ties
    want = helpers.bf16_round(f).astype(np.float64)
    assert np.array_equal(exact_ref.rne_bf16(torch.from_numpy(f.astype(np.float64))).numpy(), want)


def test_random_set_contains_the_torch_f32_result(graph):
    """TorchRef's f32 accumulation is one legal order: every stored value it produces must lie in the reference's set, and
    its f32 heads within the radius; the share of undecided outputs stays small."""
    g = graph
    rng = np.random.default_rng(1)
    wts = _Weights(g, rng, dyadic=False)
    ref, tref = exact_ref.ExactRef(g, wts), torch_ref.TorchRef(g, wts)
    n = 2
    worst, ratio = 0.0, 0.0
    for i, o in enumerate(g.ops):
        tens = _inputs(rng, g, o, n, dyadic=False)
        want = ref.run_op(i, {t: x.double() for t, x in tens.items()})
        with torch.no_grad():
            tref.run_op(i, tens)
        if o.out_b >= 0:
            first = tens[o.out] if o.out >= 0 else tens[o.out2]
            want[o.out_b] = ref.b2b_second(i, first.double())
        for t, w in want.items():
            got = _got(tens, t, w)
            if w.is_f32:
                bad, r = exact_ref.check_f32(got, w)
                ratio = max(ratio, r)
            else:
                bad, und = exact_ref.check_bf16(got, w)
                worst = max(worst, float(und.double().mean()))
            assert not bool(bad.any()), "op %d tensor %d: %d elements outside the legal set" % (i, t, int(bad.sum()))
    assert worst <= 0.10, worst
    assert 0 < ratio <= 1.0, ratio


def test_dyadic_set_is_exact_in_f32(graph):
    """On the dyadic data every f32 sum is exact: torch's f32 convs equal the f64 ones bit for bit, so TorchRef's stored bf16
    values equal RNE(v64) exactly; the sweep also meets ties-to-even both ways."""
    g = graph
    rng = np.random.default_rng(2)
    wts = _Weights(g, rng, dyadic=True)
    ref, tref = exact_ref.ExactRef(g, wts), torch_ref.TorchRef(g, wts)
    ref.radius, ref.exact = False, True
    n = 2
    ties = [0, 0]
    for i, o in enumerate(g.ops):
        tens = _inputs(rng, g, o, n, dyadic=True)
        if o.kind == 2 and o.layer2 < 0 and o.in_affine < 0:
            L = g.layers[o.layer]
            x = tens[o.in_][:, o.x_coff:o.x_coff + L.cin]
            w = torch.from_numpy(wts.w[o.layer]).permute(0, 3, 1, 2)
            a = F.conv2d(x, w, stride=L.stride, padding=L.pad)
            want64 = F.conv2d(x.double(), w.double(), stride=L.stride, padding=L.pad)
            assert torch.equal(a.double(), want64), "op %d: the f32 conv is not the exact sum (%d elements differ)" % (
                i, int((a.double() != want64).sum()))
        want = ref.run_op(i, {t: x.double() for t, x in tens.items()})
        with torch.no_grad():
            tref.run_op(i, tens)
        if o.out_b >= 0:
            first = tens[o.out] if o.out >= 0 else tens[o.out2]
            want[o.out_b] = ref.b2b_second(i, first.double())
        for t, w in want.items():
            got = _got(tens, t, w)
            assert torch.equal(w.lo, w.hi), "op %d: the dyadic set leaves an element undecided" % i
            if w.is_f32:
                c0 = 4 if w.softmax else 0
                assert torch.equal(got[:, c0:], w.v[:, c0:]), "op %d tensor %d" % (i, t)
            else:
                assert torch.equal(got, w.lo), "op %d tensor %d: %d elements differ from RNE(v64)" % (i, t, int((got != w.lo).sum()))
                d, u = exact_ref.bf16_ties(w.v)
                ties[0] += d
                ties[1] += u
    assert min(ties) >= 100, ties


@pytest.mark.parametrize("dyadic", [False, True])
def test_chunked_reference_equals_the_unchunked_one(graph, dyadic):
    """run_op / b2b_second evaluated 2 images (then 1 image: a ragged last chunk) at a time return, bit for bit, what one
    evaluation of all 5 images returns: every field of every output, on both input sets."""
    g = graph
    rng = np.random.default_rng(5)
    ref = exact_ref.ExactRef(g, _Weights(g, rng, dyadic))
    ref.radius, ref.exact = not dyadic, dyadic
    n = 5
    compared = 0
    for i, o in enumerate(g.ops):
        tens = {t: x.double() for t, x in _inputs(rng, g, o, n, dyadic).items()}
        whole = ref.run_op(i, tens)
        pairs = [(whole, ref.run_op(i, tens, chunk=2)), (whole, ref.run_op(i, tens, chunk=n)), (whole, ref.run_op(i, tens, chunk=64))]
        if o.out_b >= 0:
            first = exact_ref.rne_bf16(whole[o.out if o.out >= 0 else o.out2].v)   # what a device would have stored
            pairs.append(({0: ref.b2b_second(i, first)}, {0: ref.b2b_second(i, first, chunk=2)}))
        for a, b in pairs:
            assert a.keys() == b.keys()
            for t in a:
                assert (a[t].is_f32, a[t].softmax) == (b[t].is_f32, b[t].softmax)
                assert (a[t].dst is None) == (b[t].dst is None) and (a[t].dst is None or np.array_equal(a[t].dst, b[t].dst))
                for k in ("lo", "hi", "v", "rad"):
                    x, y = getattr(a[t], k), getattr(b[t], k)
                    assert x.shape == y.shape and x.shape[0] == n and torch.equal(x, y), "op %d tensor %d field %s" % (i, t, k)
                    compared += 1
    assert compared >= 4 * len(g.ops)
