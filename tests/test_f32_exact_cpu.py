"""tests/exact_ref_f32.py, the per-element reference of the f32 parity mode, without a GPU: every R50 op at 96x64 and 32x32
(n = 2), on stand-in weights (tests/f32_exact_cases.py).

- torch_ref.TorchRef(acc64=True).run_op -- f64 convolutions rounded once, the elementwise steps in the device's order -- is one
  legal evaluation: the reference accepts it everywhere, on both input sets;
- the check has teeth: six wrong evaluations (MUTANTS) are each rejected on at least one op; the rejected share of the elements
  of the ops a mutant touches is printed;
- the bound is not vacuous: the undecided share of every output of every op is <= 1 % on the random set and 0 on the dyadic set.
  This is a condition on the reference alone (the radius 2 K 2^-53 S against the f32 spacing 2^-24 |v|), not a measurement.

The f32 mutant sums with im2col + sgemm on every CPU (oneDNN and NNPACK off, as in tests/test_exact_ref_cpu.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_ref_f32
import f32_exact_cases
import torch_ref

GEOMETRIES = [(96, 64), (32, 32)]
N = 2


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


@pytest.fixture(scope="module", params=GEOMETRIES, ids=["%dx%d" % s for s in GEOMETRIES])
def graph(request):
    import rfd_hip
    rfd_hip.load_library()
    return rfd_hip.Graph(rfd_hip.BACKBONE_R50, *request.param)


def _got(tens, t, out):
    v = tens[t].numpy()
    return np.ascontiguousarray(v[:, out.dst] if out.dst is not None else v)


def _walk(g, wts, ref, tref, dyadic, seed, only=None):
    """every op (or those `only` accepts) on fresh inputs through tref.run_op -> [(op, tensor, bad, undecided, elements)]"""
    rng = np.random.default_rng(seed)
    rows = []
    for i, o in enumerate(g.ops):
        tens = f32_exact_cases.inputs(rng, g, o, N, dyadic)   # drawn for every op: the same data whatever `only` keeps
        if only is not None and not only(o):
            continue
        want = ref.run_op(i, tens)
        with tref.arithmetic():
            tref.run_op(i, tens)
        if o.out_b >= 0:   # as on the device: the second conv is judged from the first one's stored output
            want[o.out_b] = ref.second(i, tens[o.out] if o.out >= 0 else tens[o.out2])
        for t, w in want.items():
            bad, und, _ = exact_ref_f32.check(_got(tens, t, w), w)
            rows.append((i, t, int(bad.sum()), int(w.und.sum()), bad.size))
    return rows


@pytest.mark.parametrize("dyadic", [False, True], ids=["random", "dyadic"])
def test_acc64_walk_is_accepted_and_the_cap_holds(graph, dyadic):
    g = graph
    rng = np.random.default_rng(41)
    wts = f32_exact_cases.Weights(g, rng)
    if dyadic:
        wts.dyadic(g, rng)
    else:
        assert all(np.any(w.view(np.uint32) & 0xFFFF) for w in wts.w), "the random weights must not be bf16 values"
    ref = exact_ref_f32.ExactRefF32(g, wts)
    ref.radius, ref.exact = not dyadic, dyadic
    rows = _walk(g, wts, ref, torch_ref.TorchRef(g, wts, round_bf16=False, acc64=True), dyadic, 42)
    assert {r[0] for r in rows} == set(range(len(g.ops)))
    worst = max(r[3] / r[4] for r in rows)
    print("\nf32 exact reference %dx%d, %s set: %d outputs of %d ops, %d elements, %d undecided, worst share %.3f %%" % (
        g.tensors[g.ops[0].in_].width, g.tensors[g.ops[0].in_].height, "dyadic" if dyadic else "random", len(rows), len(g.ops),
        sum(r[4] for r in rows), sum(r[3] for r in rows), 100 * worst))
    wrong = [r for r in rows if r[2]]
    assert not wrong, "(op, tensor, bad, undecided, elements): %s" % wrong[:12]
    cap = 0.0 if dyadic else 0.01
    over = [r for r in rows if r[3] > cap * r[4]]
    assert not over, "undecided share over %.0f %%: (op, tensor, bad, undecided, elements) %s" % (100 * cap, over[:12])


# ---- wrong evaluations the reference must reject: each replaces one function torch_ref.run_op calls ----
def _conv_f32(x, w, b, stride=1, padding=0, groups=1, x2=None, w2=None, b2=None, stride2=1):
    """(a) f32 accumulation: plain F.conv2d in f32"""
    v = F.conv2d(x, w, b, stride=stride, padding=padding)
    return v if x2 is None else v + F.conv2d(x2, w2, b2, stride=stride2)


def _conv_f32_products(x, w, b, stride=1, padding=0, groups=1, x2=None, w2=None, b2=None, stride2=1):
    """(b) every product rounded to f32, then summed in f64 and rounded once (1x1 convolutions)"""
    def seg(x, w, st):
        assert w.shape[2] == w.shape[3] == 1 and padding == 0
        p = x[:, None, :, ::st, ::st] * w[None, :, :, 0, 0, None, None]   # f32 products [n][cout][cin][h][w]
        return p.double().sum(2)
    s, bias = seg(x, w, stride), b
    if x2 is not None:
        s, bias = s + seg(x2, w2, stride2), b + b2
    return s.float() + bias.view(1, -1, 1, 1)


def _conv_bias_in_f64(x, w, b, stride=1, padding=0, groups=1, x2=None, w2=None, b2=None, stride2=1):
    """(c) the bias added in f64, before the single rounding"""
    s, bias = F.conv2d(x.double(), w.double(), None, stride=stride, padding=padding), b
    if x2 is not None:
        s, bias = s + F.conv2d(x2.double(), w2.double(), None, stride=stride2), b + b2
    return (s + bias.double().view(1, -1, 1, 1)).float()


def _affine_two_roundings(x, s, t):
    """(d) the in-affine as a rounded product plus an add, not one fma"""
    return F.relu(x * s.view(1, -1, 1, 1) + t.view(1, -1, 1, 1))


def _conv_shifted(x, w, b, stride=1, padding=0, groups=1, x2=None, w2=None, b2=None, stride2=1):
    """(e) the input shifted by one pixel under the padding: columns padded p + 1 left, p - 1 right"""
    if padding > 0:
        x, padding = F.pad(x, (padding + 1, padding - 1, padding, padding)), 0
    return _ACC64_CONV(x, w, b, stride=stride, padding=padding, x2=x2, w2=w2, b2=b2, stride2=stride2)


class _TiledResidual:
    """(f) torch.nn.functional with the up-2 residual taken at (ho, wo) of the half-size map (wrapped into it) instead of
    (ho >> 1, wo >> 1)"""

    def __getattr__(self, name):
        return getattr(F, name)

    @staticmethod
    def interpolate(r, scale_factor=2, mode="nearest"):
        return r.repeat(1, 1, 2, 2)


_ACC64_CONV = torch_ref.conv
MUTANTS = [   # (name, attribute of torch_ref it replaces, replacement, ops it applies to: g -> (op -> bool))
    ("a: f32 accumulation", "conv", _conv_f32, lambda g: lambda o: True),
    ("b: products rounded to f32", "conv", _conv_f32_products, lambda g: lambda o: o.kind != 3 and g.layers[o.layer].kh == 1),
    ("c: bias added in f64", "conv", _conv_bias_in_f64, lambda g: lambda o: True),
    ("d: in-affine without fma", "affine_in", _affine_two_roundings, lambda g: lambda o: o.in_affine >= 0 or (o.kind == 6 and o.out >= 0)),
    ("e: input shifted under the padding", "conv", _conv_shifted, lambda g: lambda o: g.layers[o.layer].pad > 0),
    ("f: residual at (ho, wo)", "F", _TiledResidual(), lambda g: lambda o: o.res >= 0 and o.res_up2),
]


@pytest.mark.parametrize("mutant", MUTANTS, ids=[m[0][0] for m in MUTANTS])
def test_wrong_evaluations_are_rejected(graph, mutant, monkeypatch):
    name, attr, repl, applies = mutant
    g = graph
    rng = np.random.default_rng(41)
    wts = f32_exact_cases.Weights(g, rng)
    ref = exact_ref_f32.ExactRefF32(g, wts)
    tref = torch_ref.TorchRef(g, wts, round_bf16=False, acc64=True)
    monkeypatch.setattr(torch_ref, attr, repl)
    rows = _walk(g, wts, ref, tref, False, 42, only=applies(g))
    assert rows, "mutant %s applies to no op" % name
    bad, total = sum(r[2] for r in rows), sum(r[4] for r in rows)
    hit = sorted({r[0] for r in rows if r[2]})
    print("\nmutant %s at %dx%d: rejected on %d of %d ops, %.2f %% of %d elements" % (
        name, g.tensors[g.ops[0].in_].width, g.tensors[g.ops[0].in_].height, len(hit), len({r[0] for r in rows}), 100.0 * bad / total, total))
    assert hit, "the reference accepts mutant %s on every op" % name
