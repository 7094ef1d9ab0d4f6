"""Per-op, per-element reference of the f32 PARITY MODE (csrc/kernels_f32.hip; test infrastructure, pure torch / numpy, no GPU).

The mode's claim: a product of two f32 values is exact in f64, so every convolution output is the correctly rounded value of its
exact sum, up to the f64 summation-order noise, and everything after that one rounding is plain f32 in a fixed order.  This module
evaluates ONE op of the graph from f32 inputs (NCHW, logical channels) and the f32 weights / bias / affine the context reports,
and returns for every output element the set of f32 values the op may legally store:

- v64 = the f64 F.conv2d of all K segments in one sum, S = the same convolution of |x| with |w|, K = the term count over both
  segments.  The device and this reference each add exactly represented products in f64, in some order: each is within
  K * 2^-53 * S of the true sum (the bound has 2 * 2^-53 * S of slack, which covers the rounding of v64 -+ r itself), so
  r = 2 * K * 2^-53 * S, lo = float32(v64 - r), hi = float32(v64 + r): equal or neighbouring floats;
- the epilogue of conv_f32_kernel in numpy float32, applied to both ends in the device's order (the library is built with
  -ffp-contract=off: a * b + c is two roundings): + (bias + bias2) with the biases summed in f32 first; the residual before or
  after the ReLU, nearest-2x index (ho >> 1, wo >> 1); ReLU; out2 = relu(v * s2 + t2).  Every step is monotone (a negative scale
  swaps the ends: the ends are re-sorted after every step);
- an element is DECIDED when both ends give one value: the device must then store that value (the two zeros count as one value:
  fmaxf may return either).  An undecided element must lie between the ends.  NaN always fails;
- the in-affine operand relu(fmaf(x, s, t)): x * s is exact in f64, but (x * s + t) rounded to f64 and then to f32 can round
  twice.  With z that f64 value, the operand is undecided when float32(z (1 - 2^-52)) != float32(z (1 + 2^-52)) -- unless the
  f64 add was exact (then float32(z) is what fmaf returns, ties included); every output that reads an undecided operand is
  undecided, its interval widened by |w| times the distance of the operand's two candidates;
- with `radius=False` r is 0 (the dyadic input set: every partial sum is exact in f64 in ANY order, so the device's sum IS v64);
  `exact=True` asserts that: sum |x w| on the products' grid stays below 2^53.  Without it an exact sum of 0 would be "undecided"
  between +-r;
- the four soft-maxed score channels of a head are held by exact_ref.check_f32's rule (expf is not correctly rounded), applied to
  the logit difference as the device forms it, in f32 (Out.__init__); the box and landmark channels of the same plane are exact
  as above."""
import numpy as np
import torch
import torch.nn.functional as F

import exact_ref

U64 = 2.0 ** -53   # f64 unit round-off
F32 = np.float32


def _np32(t64):
    """f64 torch tensor -> numpy float32, one round-to-nearest-even"""
    return t64.numpy().astype(F32)


class Out:
    """One output tensor of an op, the op's own channels only (numpy float32, NCHW): the legal ends lo <= hi, `mid` = the epilogue
    of float32(v64) itself, `und` = elements with more than one legal value, `dst` = logical channel of the device tensor for
    every output channel (SSH concat slices), v64 = the f64 sum before the epilogue (torch), `score` = the exact_ref.Out that
    exact_ref.check_f32 judges the soft-maxed channels by."""

    def __init__(self, lo, hi, mid, und, v64, dst=None, softmax=False):
        self.lo, self.hi, self.mid, self.und, self.v64, self.dst, self.softmax = lo, hi, mid, und, v64, dst, softmax
        self.score = None
        if softmax:
            # The device subtracts the pair's maximum in f32 before expf: one more correctly rounded step of the fixed order, so
            # both scores of anchor a are functions of D = float32(bg - fg) alone (p_fg = sigmoid(-D), p_bg = sigmoid(D): the
            # larger logit's exponential is exactly 1).  check_f32 forms d = bg - fg in f64 from the ends it is given, so it is
            # given D's ends as "bg" and 0 as "fg".  Against the unrounded difference no f32 softmax meets its 4 ulp: half an ulp
            # of D is |D| 2^-25 relative in exp(D), 4 ulp of a small score at |D| = 4 already (the CPU's own f32 evaluation of
            # the kernel's formula: up to 10 ulp from sigmoid(bg - fg), 3.7 ulp from sigmoid(D), over 4e6 normal pairs).
            slo, shi = lo.copy(), hi.copy()
            for a in range(2):
                slo[:, a], shi[:, a] = lo[:, a] - hi[:, 2 + a], hi[:, a] - lo[:, 2 + a]   # float32 arithmetic
                slo[:, 2 + a] = shi[:, 2 + a] = 0
            d = lambda a: torch.from_numpy(a.astype(np.float64))
            self.score = exact_ref.Out(d(slo), d(shi), d(mid), (d(hi) - d(lo)) / 2, is_f32=True, softmax=True)


class _Ends:
    """(lo, hi, mid) float32 arrays through monotone f32 steps"""

    def __init__(self, lo, hi, mid):
        self.lo, self.hi, self.mid = lo, hi, mid

    def step(self, fn):
        a, b = fn(self.lo), fn(self.hi)
        return _Ends(np.minimum(a, b), np.maximum(a, b), fn(self.mid))


def _relu(a):
    return np.maximum(a, F32(0))


def _bc(c):
    return np.ascontiguousarray(c, F32).reshape(1, -1, 1, 1)


class ExactRefF32:
    def __init__(self, graph, det):
        """det: anything with get_layer(i, L) -> (w [cout][kh][kw][cin], bias) and get_affine(i, cout) -> (scale, shift), f32"""
        self.g = graph
        self.w, self.b, self.aff = [], [], []
        for i, L in enumerate(graph.layers):
            w, b = det.get_layer(i, L)
            assert w.dtype == F32 and b.dtype == F32
            self.w.append(torch.from_numpy(w).permute(0, 3, 1, 2).contiguous().double())
            self.b.append(b.copy())
            if L.has_affine:
                s, t = det.get_affine(i, L.cout)
                self.aff.append((s.astype(F32), t.astype(F32)))
            else:
                self.aff.append(None)
        self.radius = True
        self.exact = False

    # ---- the one rounded sum ----
    def _sum(self, segs, pad, dx=None):
        """segs: [(x f64, w f64, stride)], the first one padded.  -> (ends of float32(sum), v64, undecided-operand mask or None)"""
        s = S = None
        k = 0
        p = pad
        for x, w, st in segs:
            c = F.conv2d(x, w, None, stride=st, padding=p)
            a = F.conv2d(x.abs(), w.abs(), None, stride=st, padding=p)
            s, S = (c, a) if s is None else (s + c, S + a)
            k += w.shape[1] * w.shape[2] * w.shape[3]
            p = 0   # the second segment is an unpadded 1x1 conv
        if self.exact:
            e = max(exact_ref.grid_exponent(x) + exact_ref.grid_exponent(w) for x, w, _ in segs)
            assert float(S.max()) * 2.0 ** e < 2.0 ** 53, "dyadic set: sum |x w| = %g on the 2^-%d grid is not exact in f64" % (float(S.max()), e)
        r = 2.0 * k * U64 * S if self.radius else torch.zeros_like(S)
        flag = None
        if dx is not None and bool((dx > 0).any()):   # operands with two candidate values
            x, w, st = segs[0]
            r = r + F.conv2d(dx, w.abs(), None, stride=st, padding=pad)
            flag = (F.conv2d((dx > 0).double(), (w != 0).double(), None, stride=st, padding=pad) > 0).numpy()
        return _Ends(_np32(s - r), _np32(s + r), _np32(s)), s, flag

    def _operand(self, x, s, t):
        """relu(fmaf(x, s, t)) of f32 values x (f64 tensor) -> (value, distance of its two candidates: 0 where it is decided)"""
        p, t = x * torch.from_numpy(s).double().view(1, -1, 1, 1), torch.from_numpy(t).double().view(1, -1, 1, 1).expand_as(x)
        z = p + t
        a, b = (z * (1.0 - 2.0 ** -52)).float().double(), (z * (1.0 + 2.0 ** -52)).float().double()
        lo, hi = torch.minimum(a, b).clamp_min(0), torch.maximum(a, b).clamp_min(0)
        v = z.float().double().clamp_min(0)
        # where the f64 add was exact (2Sum leaves no error term) z IS x * s + t, and float32(z) what fmaf returns, ties included:
        # a short scale makes z an exact f32 tie on a whole channel, which the rule above alone would call undecided
        tt = z - p
        exact = ((p - (z - tt)) + (t - tt)) == 0
        return v, torch.where(exact, torch.zeros_like(v), hi - lo)

    @staticmethod
    def _out(e, v64, flag, nout=None, dst=None, softmax=False):
        cut = (lambda a: a) if nout is None else (lambda a: a[:, :nout])
        und = e.lo != e.hi
        if flag is not None:
            und = und | flag
        return Out(cut(e.lo), cut(e.hi), cut(e.mid), cut(und), cut(v64), dst=dst, softmax=softmax)

    # ---- ops ----
    def run_op(self, i, tens):
        """tens: dict tensor id -> NCHW float32 torch tensor (logical channels).  Returns {tensor id: Out} for every output of
        op i except out_b of a back-to-back op (second(): it reads the device's own stored first output)."""
        g = self.g
        o = g.ops[i]
        L = g.layers[o.layer]
        x = tens[o.in_].double()
        if o.kind == 3:   # stem: conv0 rounded once, + bias, ReLU (conv0_f32_kernel); 3x3/2 max-pool pad 1, mx * s + sh, ReLU
            e, v64, _ = self._sum([(x[:, :3], self.w[o.layer], 2)], 3)
            bias = _bc(self.b[o.layer])
            e = e.step(lambda a: _relu(a + bias))
            e = e.step(lambda a: F.max_pool2d(torch.from_numpy(a), 3, 2, 1).numpy())
            sc, sh = (_bc(c) for c in self.aff[o.layer])
            e = e.step(lambda a: _relu(a * sc + sh))
            return {o.out: self._out(e, v64, None)}
        assert o.kind in (2, 6), "op kind %d has no f32 kernel" % o.kind
        if x.shape[1] != L.cin:   # a channel slice of a wider tensor
            x = x[:, o.x_coff:o.x_coff + L.cin]
        dx = None
        if o.in_affine >= 0:
            x, dx = self._operand(x, *self.aff[o.in_affine])
        w, bias = self.w[o.layer], self.b[o.layer]
        if o.layer_n2 >= 0:   # sibling conv on the same input fused along N: its output channels follow
            w = torch.cat([w, self.w[o.layer_n2]], 0)
            bias = np.concatenate([bias, self.b[o.layer_n2]])
        segs = [(x, w, L.stride)]
        if o.layer2 >= 0:   # 1x1 shortcut conv as a second K segment of the same sum; the two biases are summed in f32 first
            segs.append((tens[o.in2].double(), self.w[o.layer2], g.layers[o.layer2].stride))
            bias = bias + self.b[o.layer2]
        e, v64, flag = self._sum(segs, L.pad, dx)
        bias = _bc(bias)
        e = e.step(lambda a: a + bias)
        rt = None
        if o.res >= 0:
            rt = tens[o.res].numpy().astype(F32)
            if o.res_up2:   # element (ho >> 1, wo >> 1) of the half-size map
                rt = rt.repeat(2, axis=2).repeat(2, axis=3)
            if not o.res_post:
                e = e.step(lambda a: a + rt)
        res = {}
        if o.out >= 0:
            y = e.step(_relu) if o.relu else e
            if rt is not None and o.res_post:
                y = y.step(lambda a: a + rt)
            nout = min(y.mid.shape[1], o.n_valid)
            dst = np.array([o.y_coff + n + (o.y_split_add if n >= o.y_split else 0) for n in range(nout)])
            res[o.out] = self._out(y, v64, flag, nout, dst)
        if o.out2 >= 0:
            sc, sh = (_bc(c) for c in self.aff[o.layer])
            res[o.out2] = self._out(e.step(lambda a: _relu(a * sc + sh)), v64, flag)
        if o.outf >= 0:
            res[o.outf] = self._out(e, v64, flag, softmax=bool(o.head_softmax))
        return res

    def second(self, i, first):
        """out_b of back-to-back op i: relu(conv1x1(a) + bias), a = relu(fmaf(raw, s, t)) of the device's stored raw output, or
        its stored activated output as it is when the op has no raw one.  first: NCHW float32 torch tensor of that stored tensor."""
        o = self.g.ops[i]
        a, dx = first.double(), None
        if o.out >= 0:
            a, dx = self._operand(a, *self.aff[o.layer])
        e, v64, flag = self._sum([(a, self.w[o.layer_b], 1)], 0, dx)
        bias = _bc(self.b[o.layer_b])
        return self._out(e.step(lambda v: _relu(v + bias)), v64, flag)


def check(got, out):
    """got: numpy float32 NCHW, the op's channels of the stored tensor.  Returns (bad mask, undecided mask, undecided elements
    that are not the epilogue of float32(v64)); the soft-maxed channels 0..3 of a head are judged by exact_ref.check_f32 and
    count in neither of the last two."""
    assert got.dtype == F32 and got.shape == out.lo.shape, (got.dtype, got.shape, out.lo.shape)
    bad = ~((got >= out.lo) & (got <= out.hi))   # NaN (an element never written) compares false; a decided element has lo == hi
    und = out.und.copy()
    if out.softmax:
        bad[:, :4] = exact_ref.check_f32(torch.from_numpy(got.astype(np.float64)), out.score)[0][:, :4].numpy()
        und[:, :4] = False
    off = und & ~(got == out.mid)
    return bad, und, off
